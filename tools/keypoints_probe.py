"""GPU probe: ISS keypoints and local maxima (pcgx_kdtree_iss_keypoints_dev, pcgx_kdtree_local_maxima_dev;
csrc/keypoints.hip, the eigenvalue outputs of csrc/normals.hip) against their yardsticks, all taken in the same run.

    python tools/keypoints_probe.py [--out profiles/keypoints_probe.json] [--reps 21]
    python tools/keypoints_probe.py --normals-only            (one line: normals_dev medians; for A/B with PCGX_LIB)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/keypoints_probe.py --reps 3 --kernels-only
    python tools/keypoints_probe.py --trace-summary DIR --out profiles/keypoints_probe_kernels.json

Cases: (a) synth.c4_plane(1_000_000)'s base, both radii 0.1, ~34 neighbours each (normals_probe's case); (b) a
200k-point unit cube, both radii 0.05, ~100 neighbours.  Yardsticks:
  normals_dev          the eigenvalue stage is the same kernel with other stores;
  range_count          enumerates the set the suppression kernel enumerates (host entry point: its copies are timed
                       apart and taken off, as normals_probe does; the kernels' own durations come from the trace);
  today                what a user does without this feature: RangeBatch lists on the host, then a torch segmented
                       maximum over them (scatter_reduce) and the tie-break by id.
Case (a) also times CorrespondencesDev over the keypoints' FPFH rows of the base and of the target (the base moved
and permuted): the figure the feature exists for, beside DESIGN.md 3.11's all-pairs figure at 1e5 x 1e5.
Each host figure is the median of --reps timed calls after two warm-up calls, host clock around the call and a device
synchronise."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("local_maxima_kernel", "keypoints_", "normals_kernel", "range_grid_kernel", "own_points", "fpfh_match_kernel")


def timed(fn, reps, sync):
    for _ in range(2):
        fn()
        sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "reps": reps}


def today(t, base, r, score, reps, sync, dev):
    """RangeBatch lists, then on the device: the segment maximum, and the smallest id that has it"""
    import torch
    out = {}
    lists = {}

    def ranges():
        lists["o"], lists["i"], _ = t.RangeBatch(base, r)

    out["range_batch"] = timed(ranges, reps, sync)
    n = len(base)
    offs, ids = lists["o"], lists["i"]
    d_ids = torch.from_numpy(ids).to(dev)
    d_q = torch.repeat_interleave(torch.arange(n, device=dev), torch.from_numpy(np.diff(offs)).to(dev))
    d_s = torch.from_numpy(score).to(dev)
    res = {}

    def seg():
        sj = d_s[d_ids]
        top = torch.full((n,), -float("inf"), device=dev).scatter_reduce(0, d_q, sj, "amax")
        cand = torch.where(sj == top[d_q], d_ids, torch.full_like(d_ids, n))
        first = torch.full((n,), n, dtype=torch.int64, device=dev).scatter_reduce(0, d_q, cand, "amin")
        res["ids"] = torch.nonzero((first == torch.arange(n, device=dev)) & (d_s > 0)).flatten()

    out["torch_segmented_max"] = timed(seg, reps, sync)
    out["list_entries"] = int(len(ids))
    out["maxima"] = int(len(res["ids"]))
    return out, res["ids"].cpu().numpy()


def case(name, base, r, reps, kernels_only, target=None):
    import torch
    from pcgol_amd import _lib as L
    from pcgol_amd import features, kdtree
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    t = kdtree.New(base)
    n = len(base)
    dn = torch.empty((n, 3), dtype=torch.float32, device=dev)
    de = torch.empty((n, 3), dtype=torch.float32, device=dev)
    ds = torch.empty(n, dtype=torch.float32, device=dev)
    di = torch.empty(n, dtype=torch.int32, device=dev)
    dc = torch.empty(1, dtype=torch.int32, device=dev)
    sync()
    out = {"points": n, "radius": r,
           "normals_dev": timed(lambda: t.NormalsDev(r, dn.data_ptr()), reps, sync),
           "iss_keypoints_dev": timed(lambda: t.ISSKeypointsDev(r, r, di.data_ptr(), dc.data_ptr(), de.data_ptr(),
                                                                ds.data_ptr()), reps, sync),
           "local_maxima_dev": timed(lambda: t.LocalMaximaDev(r, ds.data_ptr(), di.data_ptr(), dc.data_ptr()), reps, sync)}
    out["keypoints"] = int(dc.cpu()[0])
    sal = ds.cpu().numpy()
    out["salient_points"] = int((sal > 0).sum())
    counts = np.zeros(n, np.int64)
    qh = np.ascontiguousarray(base, np.float32)
    lib = L.lib()
    out["range_count"] = timed(lambda: L.check(lib.pcgx_kdtree_range_count(t._h, L.ptr(qh), n, r, L.ptr(counts))), reps, sync)
    out["mean_neighbours"] = float(counts.mean())
    if kernels_only:
        return out
    hq, hc = torch.from_numpy(qh.copy()), torch.from_numpy(np.empty_like(counts))
    dq2, dc2 = torch.empty_like(hq, device=dev), torch.empty_like(hc, device=dev)

    def copies():  # what range_count moves over the bus besides its kernel
        dq2.copy_(hq)
        hc.copy_(dc2)

    out["range_count_copies"] = timed(copies, reps, sync)
    out["range_count_minus_copies_ms"] = out["range_count"]["median_ms"] - out["range_count_copies"]["median_ms"]
    out["iss_minus_local_maxima_ms"] = out["iss_keypoints_dev"]["median_ms"] - out["local_maxima_dev"]["median_ms"]
    out["today"], ids_today = today(t, qh, r, sal, 3, sync, dev)
    out["today_equals_local_maxima"] = bool(np.array_equal(ids_today, di.cpu().numpy()[:out["keypoints"]]))
    if target is not None:  # the match over keypoints: the figure the feature exists for
        t2 = kdtree.New(target)
        dn2, df, df2 = torch.empty_like(dn), torch.empty((n, 33), dtype=torch.float32, device=dev), \
            torch.empty((n, 33), dtype=torch.float32, device=dev)
        di2, dc2k = torch.empty_like(di), torch.empty_like(dc)
        t.FPFHDev(r, dn.data_ptr(), df.data_ptr())
        t2.NormalsDev(r, dn2.data_ptr())
        t2.FPFHDev(r, dn2.data_ptr(), df2.data_ptr())
        t2.ISSKeypointsDev(r, r, di2.data_ptr(), dc2k.data_ptr())
        sync()  # (the library's stream is not torch's: the count below and the gathers are torch's work)
        na, nb = out["keypoints"], int(dc2k.cpu()[0])
        assert 0 < na <= n and 0 < nb <= n, (na, nb)
        fa, fb = df[di[:na].long()].contiguous(), df2[di2[:nb].long()].contiguous()
        sync()
        src, dst = torch.empty(na, dtype=torch.int32, device=dev), torch.empty(na, dtype=torch.int32, device=dev)
        cnt = torch.empty(1, dtype=torch.int32, device=dev)
        out["correspondences_over_keypoints"] = timed(
            lambda: features.CorrespondencesDev(fa.data_ptr(), na, fb.data_ptr(), nb, src.data_ptr(), dst.data_ptr(),
                                                cnt.data_ptr(), MaxRatio=1.0, Mutual=True), reps, sync)
        out["correspondences_over_keypoints"].update({"na": na, "nb": nb, "pairs": int(cnt.cpu()[0])})
    print(name, json.dumps(out), flush=True)
    return out


def normals_only(reps):
    import torch
    from pcgol_amd import kdtree, synth
    dev = torch.device("cuda", 0)
    res = {"lib": os.environ.get("PCGX_LIB", "tree")}
    for name, base, r in (("surface_1M_r0.1", synth.c4_plane(1_000_000)["base"], 0.1),
                          ("cube_200k_r0.05", synth.uniform_cloud(200_000, 1.0, 11), 0.05)):
        t = kdtree.New(base)
        dn = torch.empty((len(base), 3), dtype=torch.float32, device=dev)
        res[name] = timed(lambda: t.NormalsDev(r, dn.data_ptr()), reps, torch.cuda.synchronize)
    print(json.dumps(res), flush=True)


def trace_summary(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    by = {}
    for r in rows:
        name = r.get("Kernel_Name", "")
        if not any(s in name for s in KERNELS):
            continue
        threads = int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0)
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        by.setdefault((name, threads), []).append(us)
    out = []
    for (name, threads), v in sorted(by.items()):
        out.append({"kernel": name, "threads": threads, "dispatches": len(v), "mean_us": round(float(np.mean(v)), 2),
                    "min_us": round(float(np.min(v)), 2), "max_us": round(float(np.max(v)), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--trace-summary", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="only the library's own calls (the traced run)")
    ap.add_argument("--normals-only", action="store_true")
    a = ap.parse_args()
    if a.normals_only:
        return normals_only(a.reps)
    if a.trace_summary:
        res = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/keypoints_probe.py --reps 3 --kernels-only (no "
                      "counters in the run); durations from the trace", "kernels": trace_summary(a.trace_summary)}
    else:
        from pcgol_amd import build as B
        from pcgol_amd import synth
        res = {"source_hash": B.source_hash(), "cases": {}}
        c4 = synth.c4_plane(1_000_000)
        res["cases"]["surface_1M_r0.1"] = case("surface", c4["base"], 0.1, a.reps, a.kernels_only,
                                               None if a.kernels_only else c4["target"])
        res["cases"]["cube_200k_r0.05"] = case("cube", synth.uniform_cloud(200_000, 1.0, 11), 0.05, a.reps, a.kernels_only)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
