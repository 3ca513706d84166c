"""GPU probe: FPFH matching (pcgx_fpfh_match_dev / pcgx_fpfh_correspondences_dev, csrc/fpfh_match.hip) against two
yardsticks, neither of them the code under test:
  1. the arithmetic bound of the contract: 99 float32 vector operations per pair, none fusable, on 256 CUs x 4 SIMDs x
     16 lanes x 2.4 GHz = 39.3 T lane-operations/s unpacked, twice that if every operation issues packed;
  2. what a user does today: torch.cdist(A, B) followed by topk(2, largest=False), chunked over A so the distance
     matrix fits, on the same device in the same run.

    python tools/fpfh_match_probe.py [--out profiles/fpfh_match_probe.json] [--reps 21]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fpfh_match_probe.py --reps 3 --no-torch --no-sweep
    python tools/fpfh_match_probe.py --trace-summary DIR --out profiles/fpfh_match_probe_kernels.json

Cases: 100 000 x 100 000 and 10 000 x 1 000 000 rows built by scene R's recipe (tests/match_oracle.py).  Everything is
device resident.  Each host figure is the median of --reps timed calls after two warm-up calls, host clock around the
call and a device synchronise; the kernels' own durations come from the trace (one run, no counters).  The split sweep
times match_dev under PCGX_MATCH_SPLIT (the library's choice: unset).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9  # unpacked
OPS_PER_PAIR = 99
SWEEP = {"100k_x_100k": (1, 2, 4, 8, 16, 32, 64, 128, 256), "10k_x_1M": (32, 64, 128, 256, 512, 1024)}
KERNELS = ("fpfh_usable_kernel", "fpfh_match_kernel", "fpfh_merge_kernel", "fpfh_corr_kernel")


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


def torch_top2(dA, dB, rows):
    import torch
    out_d, out_i = [], []
    for lo in range(0, len(dA), rows):
        d, i = torch.cdist(dA[lo:lo + rows], dB).topk(2, dim=1, largest=False)
        out_d.append(d)
        out_i.append(i)
    return torch.cat(out_d), torch.cat(out_i)


def case(name, na, nb, reps, with_torch, sweep):
    import torch
    import match_oracle as MO
    from pcgol_amd import features
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    A, B = MO.scene_r(na, nb)
    dA, dB = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    ids = torch.empty(na, dtype=torch.int32, device=dev)
    d1 = torch.empty(na, dtype=torch.float32, device=dev)
    d2 = torch.empty(na, dtype=torch.float32, device=dev)
    src = torch.empty(na, dtype=torch.int32, device=dev)
    dst = torch.empty(na, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    sync()

    def match():
        features.MatchDev(dA.data_ptr(), na, dB.data_ptr(), nb, ids.data_ptr(), d1.data_ptr(), d2.data_ptr())

    def corr():
        features.CorrespondencesDev(dA.data_ptr(), na, dB.data_ptr(), nb, src.data_ptr(), dst.data_ptr(), cnt.data_ptr(),
                                    MaxRatio=0.9, Mutual=True)

    pairs = float(na) * float(nb)
    bound = pairs * OPS_PER_PAIR / LANE_OPS_PER_S * 1e3
    out = {"na": na, "nb": nb, "bound_unpacked_ms": bound, "bound_packed_ms": bound / 2,
           "match_dev": timed(match, reps, sync), "correspondences_dev_mutual": timed(corr, reps, sync)}
    out["pairs_kept"] = int(cnt.cpu()[0])
    out["match_fraction_of_packed_bound"] = out["bound_packed_ms"] / out["match_dev"]["median_ms"]
    out["match_fraction_of_unpacked_bound"] = out["bound_unpacked_ms"] / out["match_dev"]["median_ms"]
    if with_torch:
        rows = max(1, min(na, (1 << 30) // nb))  # a 4 GiB distance matrix at the most
        out["torch_cdist_topk2"] = dict(timed(lambda: torch_top2(dA, dB, rows), max(3, reps // 4), sync), chunk_rows=rows)
        out["torch_over_match"] = out["torch_cdist_topk2"]["median_ms"] / out["match_dev"]["median_ms"]
        match()
        sync()
        ti = torch_top2(dA, dB, rows)[1][:, 0].to(torch.int32)
        out["torch_same_nearest_share"] = float((ti == ids).float().mean().cpu())
    if sweep:
        out["split_sweep_match_dev"] = {}
        for s in sweep:
            os.environ["PCGX_MATCH_SPLIT"] = str(s)
            out["split_sweep_match_dev"][str(s)] = timed(match, max(5, reps // 3), sync)
        del os.environ["PCGX_MATCH_SPLIT"]
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
        grid_y = int(r.get("Grid_Size_Y", 1) or 1)  # (the chunks of B: blockIdx.y of fpfh_match_kernel)
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        by.setdefault((name, threads, grid_y), []).append(us)
    out = []
    for (name, threads, grid_y), v in sorted(by.items()):
        out.append({"kernel": name, "threads": threads, "grid_y": grid_y, "dispatches": len(v), "mean_us": round(float(np.mean(v)), 2),
                    "min_us": round(float(np.min(v)), 2), "max_us": round(float(np.max(v)), 2)})
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
        res = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/fpfh_match_probe.py --reps 3 --no-torch --no-sweep "
                      "(no counters in the run); durations from the trace", "kernels": trace_summary(a.trace_summary)}
    else:
        from pcgol_amd import build as B
        res = {"source_hash": B.source_hash(), "cases": {}}
        for name, na, nb in (("100k_x_100k", 100_000, 100_000), ("10k_x_1M", 10_000, 1_000_000)):
            res["cases"][name] = case(name, na, nb, a.reps, not a.no_torch, () if a.no_sweep else SWEEP[name])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
