"""GPU probe: pose from correspondences (pcgx_pose_from_correspondences_dev, csrc/pose.hip) against two yardsticks,
neither of them the code under test:
  1. the arithmetic bound of the contract: the unfused float32 operations per (hypothesis, pair) of mat4_transform and
     the distance as written -- w: 3 mul, 3 add, 1 div; x', y', z': 3 mul, 3 add and the mul by w each; d: 3 sub;
     DistSq: 3 mul, 2 add; 1 compare = 37 -- on 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 T lane-operations/s
     unpacked, half that time if every operation issues packed.  The count kernel leaves w out (exactly 1 under a
     status-0 pose) and executes 26 arithmetic operations, 1 compare and 1 integer add: 28; that bound is stated too.
  2. what a user does today: a batched torch evaluation of the same hypotheses' poses -- a chunked einsum of the poses
     over the source points, a squared distance, a compare-and-sum -- on the same device in the same run.

    python tools/pose_probe.py [--out profiles/pose_probe.json] [--reps 21]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pose_probe.py --reps 3 --no-torch --no-sweep
    python tools/pose_probe.py --trace-summary DIR --out profiles/pose_probe_kernels.json

Cases: 100 000 hypotheses x 10 000 pairs, 100 000 x 100 000, 4 096 x 1 500 (scene M's shape): a random cloud and its
rigidly moved copy, 40 % of the pairs with a wrong partner.  EdgeSimilarity = 0 so that every hypothesis with a proper
sample is scored (the headline: hypotheses x pairs is what the bound counts), and 0.9 beside it (most hypotheses are
rejected before they cost anything).  Everything is device resident.  Each host figure is the median of --reps timed
calls after two warm-up calls, host clock around the call and a device synchronise; the kernels' own durations come from
the trace (one run, no counters).  The split sweep times the call under PCGX_POSE_SPLIT (the library's choice: unset).
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

LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9  # unpacked
OPS_AS_WRITTEN = 37
OPS_EXECUTED = 28
CASES = (("100k_x_10k", 100_000, 10_000), ("100k_x_100k", 100_000, 100_000), ("4096_x_1500", 4096, 1500))
SWEEP = {"100k_x_10k": (1, 2, 4, 8, 16, 39, 64, 128), "100k_x_100k": (1, 4, 16, 32, 84, 128, 256, 390),
         "4096_x_1500": (1, 2, 3, 5, 8, 16, 32)}
KERNELS = ("pose_gather_kernel", "pose_fit_kernel", "pose_count_kernel", "pose_finish_kernel")


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


def scene(m, seed=1):
    rng = np.random.default_rng(seed)
    P = (rng.random((m, 3)) * 4.0).astype(np.float32)
    a = 0.7
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Q = (P.astype(np.float64) @ R.T + np.array([1.0, -2.0, 0.5])).astype(np.float32)
    src = np.arange(m, dtype=np.int32)
    dst = src.copy()
    wrong = rng.random(m) < 0.4
    dst[wrong] = rng.integers(0, m, int(wrong.sum()))
    return P, Q, src, dst


def torch_counts(poses, dP, dQ, max_dist_sq, rows):
    """counts[h] of every pose over the pairs (P[k], Q[k]): einsum, squared distance, compare-and-sum"""
    import torch
    R = poses.view(-1, 4, 4)[:, :3, :3].transpose(1, 2)  # column-major 4 x 4 -> R[h, row, col]
    t = poses.view(-1, 4, 4)[:, 3, :3]
    out = []
    for lo in range(0, len(poses), rows):
        x = torch.einsum("hij,mj->hmi", R[lo:lo + rows], dP) + t[lo:lo + rows, None, :]
        out.append((((dQ[None] - x) ** 2).sum(dim=2) < max_dist_sq).sum(dim=1))
    return torch.cat(out)


def case(name, n_hyp, m, reps, with_torch, sweep):
    import torch
    from pcgol_amd import alignment
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    P, Q, src, dst = scene(m)
    max_dist = 0.01
    dP, dQ, ds, dd = (torch.from_numpy(x).to(dev) for x in (P, Q, src, dst))
    du = torch.from_numpy(alignment.Samples(n_hyp, 7).view(np.int32)).to(dev)
    res = torch.empty(alignment.RESULT_WORDS, dtype=torch.int32, device=dev)
    ids = torch.empty(m, dtype=torch.int32, device=dev)
    st = torch.empty(n_hyp, dtype=torch.int32, device=dev)
    cn = torch.empty(n_hyp, dtype=torch.int32, device=dev)
    ps = torch.empty((n_hyp, 16), dtype=torch.float32, device=dev)
    sync()

    def run(es, refine=True):
        alignment.EstimatePoseDev(dP.data_ptr(), m, dQ.data_ptr(), m, ds.data_ptr(), dd.data_ptr(), m, du.data_ptr(), n_hyp,
                                  res.data_ptr(), max_dist, EdgeSimilarity=es, Refine=refine, d_inlier_ids=ids.data_ptr(),
                                  d_status=st.data_ptr(), d_counts=cn.data_ptr(), d_poses=ps.data_ptr())

    out = {"n_hyp": n_hyp, "m": m}
    out["edge_0.9"] = timed(lambda: run(0.9), reps, sync)
    out["edge_0.9"]["scored"] = int((st == 0).sum().cpu())
    out["edge_0.9"]["result"] = {k: (v.tolist() if hasattr(v, "tolist") else v)
                                 for k, v in alignment.ReadResult(res.cpu().numpy()).items()}
    out["edge_0"] = timed(lambda: run(0.0), reps, sync)
    scored = int((st == 0).sum().cpu())
    out["edge_0"]["scored"] = scored
    out["edge_0_no_refine"] = timed(lambda: run(0.0, False), reps, sync)
    pairs = float(scored) * float(m)
    out["bound_as_written_unpacked_ms"] = pairs * OPS_AS_WRITTEN / LANE_OPS_PER_S * 1e3
    out["bound_as_written_packed_ms"] = out["bound_as_written_unpacked_ms"] / 2
    out["bound_executed_packed_ms"] = pairs * OPS_EXECUTED / LANE_OPS_PER_S * 1e3 / 2
    out["fraction_of_packed_bound_as_written"] = out["bound_as_written_packed_ms"] / out["edge_0"]["median_ms"]
    out["fraction_of_packed_bound_executed"] = out["bound_executed_packed_ms"] / out["edge_0"]["median_ms"]
    if with_torch:
        run(0.0)
        sync()
        rows = max(1, min(n_hyp, (1 << 28) // (3 * m)))  # a 1 GiB transformed-points tensor at the most
        mds = float(np.float32(max_dist) * np.float32(max_dist))
        out["torch_einsum_count"] = dict(timed(lambda: torch_counts(ps, dP, dQ[dd.long()], mds, rows),
                                               max(3, reps // 4), sync), chunk_rows=rows)
        out["torch_over_call"] = out["torch_einsum_count"]["median_ms"] / out["edge_0"]["median_ms"]
        tc = torch_counts(ps, dP, dQ[dd.long()], mds, rows)
        ok = st == 0
        out["torch_same_count_share"] = float((tc[ok] == cn[ok]).float().mean().cpu())
    if sweep:
        out["split_sweep_edge_0"] = {}
        for s in sweep:
            os.environ["PCGX_POSE_SPLIT"] = str(s)
            out["split_sweep_edge_0"][str(s)] = timed(lambda: run(0.0), max(5, reps // 3), sync)
        del os.environ["PCGX_POSE_SPLIT"]
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
        if not any(s in name for s in KERNELS):
            continue
        threads = int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0)
        grid_y = int(r.get("Grid_Size_Y", 1) or 1)  # (the chunks of the pairs: blockIdx.y of pose_count_kernel)
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        by.setdefault((name.split("(")[0], threads, grid_y), []).append(us)
    out = []
    for (name, threads, grid_y), v in sorted(by.items()):
        out.append({"kernel": name, "threads": threads, "grid_y": grid_y, "dispatches": len(v),
                    "mean_us": round(float(np.mean(v)), 2), "min_us": round(float(np.min(v)), 2),
                    "max_us": round(float(np.max(v)), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--trace-summary", default=None)
    a = ap.parse_args()
    if a.trace_summary:
        res = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/pose_probe.py --reps 3 --no-torch "
                      "--no-sweep (no counters in the run); durations from the trace", "kernels": trace_summary(a.trace_summary)}
    else:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_resources as KR
        from pcgol_amd import build as B
        res = {"source_hash": B.source_hash(), "cases": {}}
        try:
            res["kernel_resources"] = {KR.short(k): {x: v.get(x) for x in ("VGPRs", "TotalSGPRs", "ScratchSize", "LDS Size", "Occupancy")}
                                       for k, v in KR.resources("pose.hip").items()}
        except Exception as e:  # (no compiler where the probe runs: the figures are in DESIGN.md)
            res["kernel_resources"] = "unavailable: %s" % e
        for name, n_hyp, m in CASES:
            res["cases"][name] = case(name, n_hyp, m, a.reps, not a.no_torch, () if a.no_sweep else SWEEP[name])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
