"""GPU probe: group geometry (csrc/group_stats.hip) -- GroupStatsDev chained behind ClustersDev on one stream, with the
clusters call's own time beside it, from the same process.

    python tools/group_probe.py [--out profiles/group_probe.json] [--reps 11]

Workloads: those of tools/cluster_probe.py (the 1M-point base of synth.c2_knn() at r = 0.15, and the base of
synth.c4_plane(1_000_000) at r = 0.075), Euclidean clusters.  Four calls alternate in one process:
  (a) clusters_dev               ClustersDev, every output
  (b) group_stats_dev            GroupStatsDev over (a)'s d_ids, d_sizes and d_n_clusters as they are (cap_ids =
                                 cap_groups = Len()), every output
  (c) group_stats_dev_no_obb     the same without the oriented box (no third gather)
  (d) chain                      (a) then (b), enqueued back to back, one synchronise
Each repetition times every call in turn (host clock around the call and a device synchronise, the method of
tools/cluster_probe.py), after two warm-up rounds; the figures are medians over --reps rounds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = ("clusters_dev", "group_stats_dev", "group_stats_dev_no_obb", "chain")


def workloads():
    from pcgol_amd import synth
    return [("c2_base_1M_r0.15", synth.c2_knn()["base"], 0.15), ("c4_plane_1M_r0.075", synth.c4_plane(1_000_000)["base"], 0.075)]


def measure(reps):
    import torch
    from pcgol_amd import build as B
    from pcgol_amd import kdtree
    sync = torch.cuda.synchronize
    cases = {}
    for name, base, r in workloads():
        base = np.ascontiguousarray(base[:, :3] if base.ndim == 2 else base, np.float32)
        n = len(base)
        t = kdtree.New(base)
        lab, siz, ids, cnt = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(4))
        c = torch.zeros(1, dtype=torch.int32, device="cuda")
        aabb = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        cen, cov, eig, axes, obb = (torch.empty((n, k), dtype=torch.float64, device="cuda") for k in (3, 6, 3, 9, 6))

        def clusters_dev():
            t.ClustersDev(r, lab.data_ptr(), c.data_ptr(), siz.data_ptr(), ids.data_ptr())

        def group_stats_dev(with_obb=True):
            t.GroupStatsDev(ids.data_ptr(), n, siz.data_ptr(), n, c.data_ptr(), cnt.data_ptr(), aabb.data_ptr(), cen.data_ptr(),
                            cov.data_ptr(), eig.data_ptr(), axes.data_ptr(), obb.data_ptr() if with_obb else 0)

        def chain():
            clusters_dev()
            group_stats_dev()

        calls = dict(zip(CALLS, (clusters_dev, group_stats_dev, lambda: group_stats_dev(False), chain)))
        ts = {k: [] for k in calls}
        out = {"points": n, "radius": r, "reps": reps}
        for rep in range(reps + 2):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                sync()
                if rep >= 2:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
            if rep == 0:
                g = int(c.item())
                out["clusters"] = g
                out["largest"] = siz[:3].cpu().tolist()
                out["singletons"] = int((siz[:g] == 1).sum().item())
                out["members"] = int(siz[:g].long().sum().item())
                out["counts_equal_sizes"] = bool(torch.equal(cnt[:g], siz[:g]))
                out["rows_behind_zero"] = not bool(cnt[g:].any().item() or obb[g:].any().item())
        for k, v in ts.items():
            out[k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
        out["group_stats_over_clusters"] = out["group_stats_dev"]["median_ms"] / out["clusters_dev"]["median_ms"]
        print(json.dumps({name: out}), flush=True)
        cases[name] = out
        del t
    return {"source_hash": B.source_hash(), "cases": cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    res = measure(a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
