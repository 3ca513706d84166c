"""GPU probe: minimum-distance subsampling (pcgx_kdtree_thin_dev; csrc/thin.hip) against its yardsticks, all taken in
the same run.

    python tools/thin_probe.py [--out profiles/thin_probe.json] [--reps 11]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/thin_probe.py --reps 3 --kernels-only
    python tools/thin_probe.py --trace-summary DIR --out profiles/thin_probe_kernels.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/thin_probe.py --one-call 0.1 [--score]
    python tools/thin_probe.py --trace-last-call DIR --out profiles/thin_probe_call_r0.1.json

Cases: synth.surface_cloud(1_000_000, 30, 6) (about 1100 points per square metre, spacing 0.03) at r = 0.1 (~35
neighbours) and at r = 0.03, the point spacing (~3 neighbours).  Per case:
  thin_dev hash          ThinDev with no score, with and without the owner pass, the library's default rounds;
  thin_dev curvature     ThinDev with NormalsDev's curvature as score, as many rounds as it needs (found by doubling);
  rounds                 the undecided count after R rounds for R = 1, 2, ... (ThinDev with MaxRounds = R: the state
                         after R rounds is a property of the set), until it is zero;
  local_maxima_dev       the yardstick: ONE enumeration of the same neighbourhoods plus one compaction;
  voxel_grid             the downsampler people use today, leaf = r, device form.
Each figure is the median of --reps timed calls after two warm-up calls, host clock around the call and a device
synchronise.  The per-kernel split comes from the traced run."""
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

KERNELS = ("thin_", "keypoints_", "local_maxima_kernel")


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


def case(name, pts, r, reps, kernels_only):
    import torch
    from pcgol_amd import _lib as L
    from pcgol_amd import kdtree, voxelgrid
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    t = kdtree.New(pts)
    n = len(pts)
    default = int(L.lib().pcgx_thin_default_rounds())
    dn = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dcurv = torch.empty(n, dtype=torch.float32, device=dev)
    di = torch.empty(n, dtype=torch.int32, device=dev)
    do = torch.empty(n, dtype=torch.int32, device=dev)
    dc = torch.zeros(2, dtype=torch.int32, device=dev)
    sync()
    t.NormalsDev(r, dn.data_ptr(), dcurv.data_ptr())
    sync()

    def thin(owner, score, rounds):
        t.ThinDev(r, di.data_ptr(), dc.data_ptr(), dc.data_ptr() + 4, d_owner=do.data_ptr() if owner else 0,
                  d_score=dcurv.data_ptr() if score else 0, Seed=1, MaxRounds=rounds)

    def left(score, rounds):
        thin(False, score, rounds)
        sync()
        c = dc.cpu().numpy()
        return int(c[0]), int(c[1])

    out = {"points": n, "radius": r, "default_rounds": default}
    hist = []
    for R in range(1, 4 * default + 1):
        kept, und = left(False, R)
        hist.append(und)
        if und == 0:
            break
    out["hash"] = {"rounds_run": len(hist), "undecided_after_round": hist, "kept": kept,
                   "dev": timed(lambda: thin(False, False, 0), reps, sync),
                   "dev_with_owner": timed(lambda: thin(True, False, 0), reps, sync),
                   "dev_exact_rounds": timed(lambda: thin(False, False, len(hist)), reps, sync)}
    R, probes = default, []
    while True:
        kept, und = left(True, R)
        probes.append([R, und])
        if und == 0 or R >= 16384:
            break
        R *= 2
    lo = R // 2 if len(probes) > 1 else 0  # the smallest R that finishes, by bisection between the last two probes
    hi = R
    while hi - lo > max(default // 4, 1) and und == 0:
        mid = (lo + hi) // 2
        if left(True, mid)[1] == 0:
            hi = mid
        else:
            lo = mid
    out["curvature"] = {"undecided_after_rounds": probes, "rounds_enough": hi, "kept": kept, "finished": und == 0,
                        "dev": timed(lambda: thin(False, True, hi), reps, sync),
                        "dev_with_owner": timed(lambda: thin(True, True, hi), reps, sync)}
    score = dcurv.cpu().numpy()
    host = {}

    def host_form():
        host["ids"] = t.Thin(r, Seed=1, Score=score)

    out["curvature"]["host_form"] = timed(host_form, 3, sync)
    out["local_maxima_dev"] = timed(lambda: t.LocalMaximaDev(r, dcurv.data_ptr(), di.data_ptr(), dc.data_ptr()), reps, sync)
    lm = out["local_maxima_dev"]["median_ms"]
    out["hash"]["ratio_to_local_maxima"] = out["hash"]["dev"]["median_ms"] / lm
    out["hash"]["with_owner_ratio_to_local_maxima"] = out["hash"]["dev_with_owner"]["median_ms"] / lm
    out["curvature"]["ratio_to_local_maxima"] = out["curvature"]["dev"]["median_ms"] / lm
    if not kernels_only:
        # (the reference sizes its dense grid by the cloud's maximum, not its extent, voxelgrid.go:46: a cloud with
        # negative coordinates does not fit, so the filter gets the cloud moved to the origin)
        moved = np.ascontiguousarray(pts - pts.min(axis=0), np.float32)
        d_in = torch.from_numpy(moved).to(dev)
        d_out = torch.empty_like(d_in)
        vg = voxelgrid.New([r, r, r])
        res = {}

        def voxel():
            res["m"] = vg.FilterDev(d_in.data_ptr(), n, 12, 0, d_out.data_ptr())

        out["voxel_grid_leaf_r"] = timed(voxel, reps, sync)
        out["voxel_grid_leaf_r"]["points_out"] = int(res["m"])
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
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        by.setdefault(name.split("(")[0], []).append(us)
    out = []
    for name, v in sorted(by.items()):
        out.append({"kernel": name, "dispatches": len(v), "total_us": round(float(np.sum(v)), 1),
                    "mean_us": round(float(np.mean(v)), 2), "min_us": round(float(np.min(v)), 2),
                    "max_us": round(float(np.max(v)), 2)})
    return out


def one_call(r, score):
    """warm-up calls, then ONE ThinDev with owners and nothing behind it: the traced run whose last call
    --trace-last-call lists dispatch by dispatch"""
    import torch
    from pcgol_amd import kdtree, synth
    dev = torch.device("cuda", 0)
    pts = synth.surface_cloud(1_000_000, 30.0, 6)[0]
    t = kdtree.New(pts)
    n = len(pts)
    dn = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dcurv = torch.empty(n, dtype=torch.float32, device=dev)
    di, do = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    dc = torch.zeros(2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t.NormalsDev(r, dn.data_ptr(), dcurv.data_ptr())
    for _ in range(3):
        torch.cuda.synchronize()
        t.ThinDev(r, di.data_ptr(), dc.data_ptr(), dc.data_ptr() + 4, d_owner=do.data_ptr(),
                  d_score=dcurv.data_ptr() if score else 0, Seed=1)
    torch.cuda.synchronize()
    print(json.dumps({"radius": r, "score": bool(score), "kept": int(dc.cpu()[0]), "left": int(dc.cpu()[1])}))


def trace_last_call(d):
    """the dispatches from the last thin_prep_kernel on, in start order: one ThinDev call, round by round"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    last = max(k for k, r in enumerate(rows) if "thin_prep_kernel" in r["Kernel_Name"])
    rows = rows[last:]
    t0, t1 = int(rows[0]["Start_Timestamp"]), max(int(r["End_Timestamp"]) for r in rows)
    us = [(r["Kernel_Name"].split("(")[0].replace("void ", "").replace("pcgx::", ""),
           (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows]
    rounds, other = [], []
    for name, v in us:
        if name.startswith("thin_round_kernel"):
            rounds.append({"round_us": round(v, 2), "commit_scan_write_us": 0.0})
        elif name in ("thin_commit_kernel", "thin_scan_kernel", "thin_write_kernel"):
            rounds[-1]["commit_scan_write_us"] = round(rounds[-1]["commit_scan_write_us"] + v, 2)
        else:
            other.append({"kernel": name, "us": round(v, 2)})
    busy = sum(v for _, v in us)
    return {"dispatches": len(us), "span_us": round((t1 - t0) / 1e3, 1), "kernels_busy_us": round(busy, 1),
            "between_kernels_us": round((t1 - t0) / 1e3 - busy, 1),
            "round_kernels_us": round(sum(x["round_us"] for x in rounds), 1),
            "commit_scan_write_us": round(sum(x["commit_scan_write_us"] for x in rounds), 1), "rounds": rounds, "other": other}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--trace-summary", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="only the library's own calls (the traced run)")
    ap.add_argument("--one-call", type=float, default=None, help="radius: warm-up, then one ThinDev with owners (traced)")
    ap.add_argument("--score", action="store_true", help="with --one-call: the curvature as score")
    ap.add_argument("--trace-last-call", default=None)
    a = ap.parse_args()
    if a.one_call is not None:
        return one_call(a.one_call, a.score)
    if a.trace_last_call:
        res = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/thin_probe.py --one-call R "
                      "(no counters in the run): the last ThinDev call of the run, with owners, dispatch by dispatch",
               "last_call": trace_last_call(a.trace_last_call)}
    elif a.trace_summary:
        res = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/thin_probe.py --reps 3 "
                      "--kernels-only (no counters in the run); durations from the trace, every dispatch of the run",
               "kernels": trace_summary(a.trace_summary)}
    else:
        from pcgol_amd import build as B
        from pcgol_amd import synth
        res = {"source_hash": B.source_hash(), "cases": {}}
        pts = synth.surface_cloud(1_000_000, 30.0, 6)[0]
        res["cases"]["surface_1M_r0.1"] = case("r0.1", pts, 0.1, a.reps, a.kernels_only)
        res["cases"]["surface_1M_r0.03"] = case("r0.03", pts, 0.03, a.reps, a.kernels_only)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
