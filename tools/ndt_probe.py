"""GPU probe: NDT registration (csrc/ndt.hip) -- map creation, one evaluation at 1, 7 and 27 candidate voxels, a
20-iteration Fit -- with pcgx_icp_gicp_fit on the same clouds beside it as the yardstick, from the same process.

    python tools/ndt_probe.py [--out profiles/ndt_probe.json] [--reps 11]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ndt_probe.py --reps 3
    python tools/ndt_probe.py --trace-summary DIR --out profiles/ndt_probe.json     (adds "kernel_trace" to the file)

Workload: the base of synth.c4_plane(1_000_000) (1M surface points, width 30) as the map at resolution 1.0 (grid
33 x 33 x 5 from (-1, -1, -2)), its target (the base permuted and moved by synth.icp_pose()) as the moved cloud.  The
calls alternate in one process: each repetition times every call in turn (host clock around the call and a device
synchronise, the method of tools/mls_probe.py), after two warm-up rounds; the figures are medians over --reps rounds.
The evaluations are device resident (pcgx_ndt_evaluate_dev); map creation and both Fits take host arrays and include
their uploads.  The GICP Fit is given covariances computed beforehand (k = 20, PLANE), which are not timed.
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

KERNELS = ("ndt_", "icp_gicp_sums_kernel", "icp_corr", "icp_grid")


def measure(reps):
    import torch
    from pcgol_amd import build as B
    from pcgol_amd import icp, kdtree, ndt, segmentation, synth
    c = synth.c4_plane(1_000_000)
    base, target = c["base"], c["target"]
    sync = torch.cuda.synchronize
    vg = segmentation.StorageVoxelGrid(1.0, (33, 33, 5), (-1.0, -1.0, -2.0))
    vg.AddAll(base)
    m = ndt.NDTMap(vg, base)
    dt = torch.from_numpy(target).cuda()
    ds = torch.zeros(30, dtype=torch.float64, device="cuda")
    th = np.full(6, -1, np.float32)
    reg = ndt.NDT(m, Threshold=th, MaxIteration=20)
    tree = kdtree.New(base)
    bcov = tree.Covariances(20)[0]
    tcov = kdtree.New(target).Covariances(20)[0]
    gicp = icp.GeneralizedICP(icp.GeneralizedICPEvaluator(icp.NearestPointCorresponder(c["max_dist"]), bcov, tcov),
                              icp.GaussNewtonUpdaterFactory(Threshold=th, MaxIteration=20))
    sync()
    results = {}

    def fit_ndt():
        results["ndt"] = reg.Fit(target)

    def fit_gicp():
        results["gicp"] = gicp.Fit(tree, target)

    calls = {
        "map_create": lambda: ndt.NDTMap(vg, base),
        "evaluate_dev_1": lambda: m.EvaluateDev(dt, ds, None, 1),
        "evaluate_dev_7": lambda: m.EvaluateDev(dt, ds, None, 7),
        "evaluate_dev_27": lambda: m.EvaluateDev(dt, ds, None, 27),
        "ndt_fit_20": fit_ndt,
        "gicp_fit_20": fit_gicp,
    }
    ts = {k: [] for k in calls}
    for rep in range(reps + 2):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            sync()
            if rep >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    occupied, valid = m.Counts()
    out = {"base_points": len(base), "target_points": len(target), "resolution": 1.0, "grid": [33, 33, 5],
           "occupied_voxels": occupied, "valid_voxels": valid, "reps": reps}
    for k, v in ts.items():
        out[k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
    inv = np.linalg.inv(synth.icp_pose().astype(np.float64).reshape(4, 4).T).T.reshape(-1)
    for k in ("ndt", "gicp"):
        trans, stat = results[k]
        out[k + "_iterations"] = int(stat.NumIteration)
        out[k + "_pose_error_max"] = float(np.max(np.abs(trans.astype(np.float64) - inv)))
    s = m.Evaluate(target[:100000], None, 7)
    out["pairs_per_point_7"] = float(s[29]) / 100000.0
    out["ndt_fit_over_gicp_fit"] = out["ndt_fit_20"]["median_ms"] / out["gicp_fit_20"]["median_ms"]
    print(json.dumps(out), flush=True)
    return {"source_hash": B.source_hash(), "cases": {"c4_plane_1M_res1.0": out}}


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
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        by.setdefault(name.split("(")[0], []).append(us)
    out = []
    for name, v in sorted(by.items()):
        out.append({"kernel": name, "dispatches": len(v), "median_us": round(float(np.median(v)), 2),
                    "min_us": round(float(np.min(v)), 2), "max_us": round(float(np.max(v)), 2)})
    return {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/ndt_probe.py --reps 3 (no counters "
                   "in the run); durations from the trace", "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--trace-summary", default=None)
    a = ap.parse_args()
    if a.trace_summary:
        res = {}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        res["kernel_trace"] = trace_summary(a.trace_summary)
    else:
        res = measure(a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
