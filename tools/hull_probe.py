"""GPU probe: group footprints (csrc/group_hull.hip) -- GroupHullsDev chained behind ClustersDev on one stream, beside
GroupStatsDev and the clusters call measured in the same run, and the time of each stage of one GroupHullsDev call.

    python tools/hull_probe.py [--out profiles/hull_probe.json] [--reps 11]

Workloads: the two of tools/group_probe.py (the 1M-point base of synth.c2_knn() at r = 0.15, and the base of
synth.c4_plane(1_000_000) at r = 0.075), and a third of many small clusters: synth.uniform_cloud(1_000_000, 1.0, 73) at
r = 0.006.  Four calls alternate in one process:
  (a) clusters_dev       ClustersDev, every output
  (b) group_stats_dev    GroupStatsDev over (a)'s d_ids, d_sizes and d_n_clusters as they are, every output
  (c) group_hulls_dev    GroupHullsDev over the same, every output
  (d) chain              (a) then (c), enqueued back to back, one synchronise
Each repetition times every call in turn (host clock around the call and a device synchronise, the method of
tools/group_probe.py), after two warm-up rounds; the figures are medians over --reps rounds.  There is no threshold.
Stages: one more GroupHullsDev call under torch.profiler, the device time of its kernels summed by stage (by kernel
name; "sort" is radix_sort_pairs' kernels and the key gathers between its passes, over the capacity).  Where the
profiler gives no kernel times, "stages" is null and says why.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = ("clusters_dev", "group_stats_dev", "group_hulls_dev", "chain")
STAGES = (("offsets_map", ("gs_tile_sum", "gs_tile_scan", "gh_offsets", "gs_map")), ("extremes", ("gh_extreme",)),
          ("filter", ("gh_filter",)), ("sort", ("gh_key", "rs_")), ("compaction", ("gh_head", "gh_flag")),
          ("reduce", ("gh_reduce",)), ("chain", ("gh_bounds", "gh_chain")), ("finish", ("gh_write", "gh_rect")))


def workloads():
    from pcgol_amd import synth
    return [("c2_base_1M_r0.15", synth.c2_knn()["base"], 0.15), ("c4_plane_1M_r0.075", synth.c4_plane(1_000_000)["base"], 0.075),
            ("uniform_1M_r0.006", synth.uniform_cloud(1_000_000, 1.0, 73), 0.006)]


def stage_times(fn):
    """-> {stage: ms} of the kernels of one call of fn, or a string saying why not"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0)))
                for e in prof.key_averages()]
    except Exception as e:  # (a build of torch without the device tracer)
        return "torch.profiler: %s" % e
    out = {name: 0.0 for name, _ in STAGES}
    out["other"] = 0.0
    seen = False
    for key, us in rows:
        if us <= 0.0 or not ("gh_" in key or "gs_" in key or "rs_" in key or "Memset" in key or "memset" in key):
            continue
        seen = seen or "gh_" in key
        for name, pats in STAGES:
            if any(p in key for p in pats):
                out[name] += us / 1e3
                break
        else:
            out["other"] += us / 1e3
    return out if seen else "torch.profiler recorded no kernel of the call"


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
        lab, siz, ids, cnt, hs, hid = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(6))
        c = torch.zeros(1, dtype=torch.int32, device="cuda")
        aabb = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        cen, cov, eig, axes, obb, rect = (torch.empty((n, k), dtype=torch.float64, device="cuda") for k in (3, 6, 3, 9, 6, 6))
        area = torch.empty(n, dtype=torch.float64, device="cuda")

        def clusters_dev():
            t.ClustersDev(r, lab.data_ptr(), c.data_ptr(), siz.data_ptr(), ids.data_ptr())

        def group_stats_dev():
            t.GroupStatsDev(ids.data_ptr(), n, siz.data_ptr(), n, c.data_ptr(), cnt.data_ptr(), aabb.data_ptr(), cen.data_ptr(),
                            cov.data_ptr(), eig.data_ptr(), axes.data_ptr(), obb.data_ptr())

        def group_hulls_dev():
            t.GroupHullsDev(ids.data_ptr(), n, siz.data_ptr(), n, c.data_ptr(), hs.data_ptr(), hid.data_ptr(), area.data_ptr(),
                            rect.data_ptr())

        def chain():
            clusters_dev()
            group_hulls_dev()

        calls = dict(zip(CALLS, (clusters_dev, group_stats_dev, group_hulls_dev, chain)))
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
                out["hull_vertices"] = int(hs[:g].long().sum().item())
                out["largest_hulls"] = hs[:3].cpu().tolist()
                out["singleton_hulls_are_one"] = bool((hs[:g][siz[:g] == 1] == 1).all().item())
                out["rows_behind_zero"] = not bool(hs[g:].any().item() or rect[g:].any().item())
                # a hull reaches its group's x and y extremes: GroupStats over the hulls gives the same xy box
                box = aabb.clone()
                t.GroupStatsDev(hid.data_ptr(), n, hs.data_ptr(), n, c.data_ptr(), 0, aabb.data_ptr())
                sync()
                out["hull_boxes_equal_group_boxes"] = bool(torch.equal(box[:g][:, [0, 1, 3, 4]], aabb[:g][:, [0, 1, 3, 4]]))
        for k, v in ts.items():
            out[k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
        out["group_hulls_over_group_stats"] = out["group_hulls_dev"]["median_ms"] / out["group_stats_dev"]["median_ms"]
        out["group_hulls_over_clusters"] = out["group_hulls_dev"]["median_ms"] / out["clusters_dev"]["median_ms"]
        out["stages_ms"] = stage_times(group_hulls_dev)
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
