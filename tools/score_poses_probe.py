"""GPU probe: K poses scored on the whole clouds in one call (pcgx_kdtree_score_poses_dev; csrc/pose_score.hip) against
what a caller does without it: per pose a torch transform, NearestBatchDev with PCGX_KNN_PRESORT, a torch count and sum.

    python tools/score_poses_probe.py [--out profiles/score_poses_probe.json] [--reps 21]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/score_poses_probe.py --reps 3 --kernels-only
    python tools/score_poses_probe.py --trace-summary DIR --out profiles/score_poses_probe_kernels.json

Workload: the tree over synth.c4_plane(1_000_000)'s base, the source its moved copy (the benchmark's ICP target), K = 16
poses: the pose that takes the copy back, its translation stepped along x from 0 to 0.05; max_dist the ICP benchmark's.
The method is tools/fpfh_at_probe.py's: everything device resident, host clock around the call plus a device
synchronise, two warm-up rounds, the median and min-max of --reps timed rounds, the yardstick and the new call
alternating (A B A B ...) in one process on one stream.  Counts are asserted equal in the same run."""
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

KERNELS = ("score_", "grid_nearest", "nearest_kernel", "qp_", "rs_", "radix", "minmax", "morton")
K_POSES, STEP_TO = 16, 0.05


def stats(ts):
    ts = np.asarray(ts)
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()),
            "q1_ms": float(np.percentile(ts, 25)), "q3_ms": float(np.percentile(ts, 75)), "reps": int(len(ts))}


def alternate(fa, fb, reps, sync):
    """A B A B ...: two warm-up rounds, then `reps` timed rounds -> (stats of A, stats of B)"""
    ta, tb = [], []
    for k in range(reps + 2):
        for fn, ts in ((fa, ta), (fb, tb)):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if k >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ta), stats(tb)


def poses_for(T):
    """the inverse of the rigid T (float64, rounded once), its translation stepped along x"""
    M = np.asarray(T, np.float64).reshape(4, 4).T
    R, t = M[:3, :3], M[:3, 3]
    Ri, ti = R.T, -R.T @ t
    out = np.zeros((K_POSES, 16), np.float32)
    for k in range(K_POSES):
        m = np.eye(4)
        m[:3, :3] = Ri
        m[:3, 3] = ti + np.array([STEP_TO * k / (K_POSES - 1), 0.0, 0.0])
        out[k] = m.T.reshape(-1).astype(np.float32)
    return out


def run(reps, kernels_only):
    import torch
    from pcgol_amd import alignment, kdtree, synth
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    c4 = synth.c4_plane(1_000_000)
    n, max_dist = len(c4["target"]), float(c4["max_dist"])
    tree = kdtree.New(c4["base"])
    poses = poses_for(synth.icp_pose())
    dP = torch.from_numpy(np.ascontiguousarray(c4["target"], np.float32)).to(dev)
    dM = torch.from_numpy(poses).to(dev)
    Rt = [torch.from_numpy(np.ascontiguousarray(m.reshape(4, 4)[:3, :3])).to(dev) for m in poses]  # (column-major: R^T)
    tt = [torch.from_numpy(m[12:15].copy()).to(dev) for m in poses]
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    dsq = torch.empty(n, dtype=torch.float32, device=dev)
    yc = torch.zeros(K_POSES, dtype=torch.int64, device=dev)
    ys = torch.zeros(K_POSES, dtype=torch.float64, device=dev)
    nc = torch.zeros(K_POSES, dtype=torch.int32, device=dev)
    ns = torch.zeros(K_POSES, dtype=torch.float64, device=dev)
    res = torch.zeros(alignment.RESULT_WORDS, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()  # torch's kernels and the library's in one queue
    torch.cuda.set_stream(stream)

    def yardstick():
        st = torch.cuda.current_stream().cuda_stream
        for k in range(K_POSES):
            x = torch.addmm(tt[k], dP, Rt[k])
            tree.NearestBatchDev(x.data_ptr(), n, max_dist, ids.data_ptr(), dsq.data_ptr(), presort=True, stream=st)
            hit = ids >= 0
            yc[k] = hit.sum()
            ys[k] = torch.where(hit, dsq, torch.zeros_like(dsq)).sum(dtype=torch.float64)

    def fused():
        alignment.ScorePosesDev(tree, dP.data_ptr(), n, dM.data_ptr(), K_POSES, max_dist, res.data_ptr(),
                                d_counts=nc.data_ptr(), d_sums=ns.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)

    sy, sf = alternate(yardstick, fused, reps, sync)
    hy, hn = yc.cpu().numpy(), nc.cpu().numpy().astype(np.int64)
    assert np.array_equal(hy, hn), (hy.tolist(), hn.tolist())
    rel = np.abs(ys.cpu().numpy() - ns.cpu().numpy()) / np.maximum(ys.cpu().numpy(), 1e-300)
    rec = alignment.ReadScore(res.cpu().numpy())
    out = {"points": n, "tree_points": len(c4["base"]), "poses": K_POSES, "max_dist": max_dist, "translation_step_to": STEP_TO,
           "per_pose_transform_nearest_count": sy, "score_poses_dev": sf, "counts": hn.tolist(), "counts_equal": True,
           "sums": ns.cpu().numpy().tolist(), "sums_max_relative_difference": float(rel.max()),
           "best": rec["best"], "best_count": rec["best_count"],
           "fused_faster_by_ms": sy["median_ms"] - sf["median_ms"],
           "faster_beyond_spread": bool(sf["max_ms"] < sy["min_ms"]),
           "slower_beyond_spread": bool(sf["min_ms"] > sy["max_ms"])}
    if kernels_only:
        out = {"traced": True, "reps": reps}
    print(json.dumps(out), flush=True)
    return out


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
        by.setdefault((name.split("(")[0], threads), []).append(us)
    out = []
    for (name, threads), v in sorted(by.items()):
        out.append({"kernel": name, "threads": threads, "dispatches": len(v), "median_us": round(float(np.median(v)), 2),
                    "min_us": round(float(np.min(v)), 2), "max_us": round(float(np.max(v)), 2),
                    "total_us": round(float(np.sum(v)), 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--trace-summary", default=None, metavar="DIR")
    ap.add_argument("--kernels-only", action="store_true", help="the two calls only (the traced run)")
    a = ap.parse_args()
    if a.trace_summary:
        res = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/score_poses_probe.py --reps 3 "
                      "--kernels-only (one run, no counters); durations from the trace, 5 rounds of each call",
               "kernels": trace_summary(a.trace_summary)}
    else:
        from pcgol_amd import build as B
        res = {"source_hash": B.source_hash(), "result": run(a.reps, a.kernels_only)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
