"""GPU probe: k nearest neighbours (pcgx_kdtree_knearest_dev, csrc/knearest.hip) against pcgx_kdtree_range_count on
the same queries at the radius whose mean count is about k -- the yardstick: it enumerates a neighbourhood of the
same size, without keeping a sorted top k.

    python tools/knearest_probe.py [--out profiles/knearest_probe.json] [--reps 21]
    python tools/knearest_probe.py --trace-summary DIR --out profiles/knearest_probe_kernels.json

Cases: (a) the 1M-point synth.surface_cloud of width 30 (C4's plane scene), q == NULL (the tree's own points), k = 16;
(b) 200k random queries in a 200k-point unit-cube cloud, k = 16; each on the grid, (a) also on the forced tree walk
(PCGX_RANGE_WALK=1).  The range radius is found from one counting pass (mean count scales with r^2 on the surface,
r^3 in the cube).  Each figure is the median of --reps timed calls after two warm-up calls, host clock around the call
and a device synchronise.  knearest_dev is device resident; range_count is the host entry point, so the copies it
makes (queries up, int64 counts down, timed with torch) are listed apart to give the kernel-side comparison.
--trace-summary reads the kernel_trace.csv files of a `rocprofv3 --kernel-trace --stats` run of this probe (no
counters) and writes per-kernel durations.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def case(name, base, queries, k, r0, dim, reps, walk=False):
    import torch
    from pcgol_amd import _lib as L
    from pcgol_amd import kdtree
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    if walk:
        os.environ["PCGX_RANGE_WALK"] = "1"
    try:
        t = kdtree.New(base)
        own = queries is None
        q = base if own else queries
        nq = len(q)
        qh = np.ascontiguousarray(q, dtype=np.float32)
        lib = L.lib()
        counts = np.zeros(nq, np.int64)
        # the radius whose mean count is about k
        L.check(lib.pcgx_kdtree_range_count(t._h, L.ptr(qh), nq, r0, L.ptr(counts)))
        r = float(r0 * (k / max(counts.mean(), 1e-9)) ** (1.0 / dim))
        dq = None if own else torch.from_numpy(qh).to(dev)
        di = torch.empty((nq, k), dtype=torch.int32, device=dev)
        dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
        sync()

        def knearest():
            L.check(lib.pcgx_kdtree_knearest_dev(t._h, None if own else C.c_void_p(dq.data_ptr()), nq, k,
                                                 float("inf"), C.c_void_p(di.data_ptr()), C.c_void_p(dd.data_ptr()),
                                                 None, None))

        def range_count():
            L.check(lib.pcgx_kdtree_range_count(t._h, L.ptr(qh), nq, r, L.ptr(counts)))

        hq = torch.from_numpy(qh.copy())
        hc = torch.from_numpy(np.empty_like(counts))
        dq2 = torch.empty_like(hq, device=dev)
        dc2 = torch.empty_like(hc, device=dev)

        def copies():  # what range_count moves over the bus besides its kernel
            dq2.copy_(hq)
            hc.copy_(dc2)

        out = {"points": len(base), "queries": nq, "own_points": own, "k": k, "walk_forced": walk,
               "knearest_dev": timed(knearest, reps, sync), "range_count": timed(range_count, reps, sync),
               "range_count_copies": timed(copies, reps, sync), "range_radius": r}
        out["range_mean_count"] = float(counts.mean())
        kern = out["range_count"]["median_ms"] - out["range_count_copies"]["median_ms"]
        out["range_count_minus_copies_ms"] = kern
        out["knearest_over_range_count_kernel"] = out["knearest_dev"]["median_ms"] / kern if kern > 0 else None
        print(name, json.dumps(out), flush=True)
        return out
    finally:
        os.environ.pop("PCGX_RANGE_WALK", None)


def trace_summary(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    by = {}
    for r in rows:
        name = r.get("Kernel_Name", "")
        if not any(s in name for s in ("knearest", "range_", "morton", "knn_own", "sor_", "grid_", "build", "radix")):
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
    a = ap.parse_args()
    if a.trace_summary:
        res = {"how": "rocprofv3 --kernel-trace --stats -- python tools/knearest_probe.py --reps 3 and "
                      "python tools/sor_probe.py --reps 3 (no counters in the run); durations from the trace",
               "kernels": trace_summary(a.trace_summary)}
    else:
        from pcgol_amd import build as B
        from pcgol_amd import synth
        res = {"source_hash": B.source_hash(), "cases": {}}
        surf = synth.surface_cloud(1_000_000, 30.0, 6)[0]
        res["cases"]["surface_1M_own_k16"] = case("surface", surf, None, 16, 0.1, 2, a.reps)
        res["cases"]["surface_1M_own_k16_walk"] = case("surface_walk", surf, None, 16, 0.1, 2, a.reps, walk=True)
        res["cases"]["cube_200k_queries_k16"] = case("cube", synth.uniform_cloud(200_000, 1.0, 11),
                                                     synth.uniform_cloud(200_000, 1.0, 14), 16, 0.05, 3, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
