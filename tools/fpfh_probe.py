"""GPU probe: FPFH descriptors (pcgx_kdtree_fpfh_dev, csrc/fpfh.hip) against pcgx_kdtree_normals_dev(q == NULL) on
the same tree and radius in the same run -- the yardstick: it makes the same enumeration once, with less work per hit.

    python tools/fpfh_probe.py [--out profiles/fpfh_probe.json] [--reps 21]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/fpfh_probe.py --reps 3
    python tools/fpfh_probe.py --trace-summary DIR --out profiles/fpfh_probe_kernels.json

Cases: (a) synth.c4_plane(1_000_000)'s base, r = 0.1, ~34 neighbours each (normals_probe's case), with its analytic
normals; (b) a 200k-point unit cube, r = 0.05, ~100 neighbours, with seeded random unit normals.  Everything is device
resident.  Each host figure is the median of --reps timed calls after two warm-up calls, host clock around the call
and a device synchronise; the two kernels' own durations come from the trace (one run, no counters).
"""
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


def case(name, base, normals, r, reps):
    import torch
    from pcgol_amd import kdtree
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    t = kdtree.New(base)
    n = len(base)
    dn = torch.from_numpy(np.ascontiguousarray(normals, np.float32)).to(dev)
    dn2 = torch.empty((n, 3), dtype=torch.float32, device=dev)
    df = torch.empty((n, 33), dtype=torch.float32, device=dev)
    dm = torch.empty(n, dtype=torch.int32, device=dev)
    sync()
    out = {"points": n, "radius": r,
           "fpfh_dev": timed(lambda: t.FPFHDev(r, dn.data_ptr(), df.data_ptr(), 0, dm.data_ptr()), reps, sync),
           "normals_dev": timed(lambda: t.NormalsDev(r, dn2.data_ptr()), reps, sync)}
    out["mean_valid_pairs"] = float(dm.cpu().numpy().mean())
    out["fpfh_over_normals"] = out["fpfh_dev"]["median_ms"] / out["normals_dev"]["median_ms"]
    print(name, json.dumps(out), flush=True)
    return out


def trace_summary(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    by = {}
    for r in rows:
        name = r.get("Kernel_Name", "")
        if not any(s in name for s in ("spfh_kernel", "fpfh_kernel", "normals_kernel", "own_points")):
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
        res = {"how": "rocprofv3 --kernel-trace --stats -- python tools/fpfh_probe.py --reps 3 (no counters in the "
                      "run); durations from the trace", "kernels": trace_summary(a.trace_summary)}
    else:
        from pcgol_amd import build as B
        from pcgol_amd import synth
        res = {"source_hash": B.source_hash(), "cases": {}}
        c4 = synth.c4_plane(1_000_000)
        res["cases"]["surface_1M_r0.1"] = case("surface", c4["base"], c4["normals"], 0.1, a.reps)
        v = np.random.default_rng(42).standard_normal((200_000, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        res["cases"]["cube_200k_r0.05"] = case("cube", synth.uniform_cloud(200_000, 1.0, 11), v, 0.05, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
