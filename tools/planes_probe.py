"""GPU probe: plane segmentation (csrc/planes.hip) -- PlanesDev on a 1M-point scene at n_hyp 256 and 1024, max_planes 1
and 4, with and without normals, Refine on and off.

    python tools/planes_probe.py [--out profiles/planes_probe.json] [--reps 11] [--only NAME]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/planes_probe.py --reps 3 --only NAME
    python tools/planes_probe.py --trace-summary DIR --out profiles/planes_probe.json   (adds "kernel_trace" to the file)

Workload: the base of synth.c4_plane(600_000) (a gently waved ground, 23 m wide) plus two walls of 200 000 and 150 000
points and 50 000 clutter points, shuffled; normals: the ground's analytic ones, the walls' own, random ones for the
clutter.  max_dist 0.25, min_inliers 50 000.  The calls (hN_pM[_n][_r]: N hypotheses, M planes, with normals, refined)
alternate in one process; each repetition times every call in turn (host clock around the call and a device
synchronise, the method of tools/dbscan_probe.py) after two warm-up rounds; the figures are medians over --reps rounds.
The trace summary sums the kernels of a run by name (run it with --only: one kind of call in the trace); the count
kernel's rate is point-hypotheses per second over its launches that did work (longer than 20 us)."""
import argparse
import csv
import glob
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_DIST, MIN_INLIERS = 0.25, 50_000


def scene():
    from pcgol_amd import synth
    c = synth.c4_plane(600_000)
    rng = np.random.default_rng(17)
    w = 30.0 * 0.6 ** 0.5
    wall_a = np.column_stack([np.full(200_000, 0.0) + rng.normal(0, 0.01, 200_000), rng.random(200_000) * w,
                              rng.random(200_000) * 6 + 1])
    wall_b = np.column_stack([rng.random(150_000) * w, np.full(150_000, w) + rng.normal(0, 0.01, 150_000),
                              rng.random(150_000) * 6 + 1])
    clutter = rng.random((50_000, 3)) * (w, w, 7)
    P = np.concatenate([c["base"], wall_a, wall_b, clutter]).astype(np.float32)
    r = rng.standard_normal((50_000, 3))
    M = np.concatenate([c["normals"], np.tile([1.0, 0, 0], (200_000, 1)), np.tile([0, 1.0, 0], (150_000, 1)),
                        r / np.linalg.norm(r, axis=1)[:, None]]).astype(np.float32)
    p = rng.permutation(len(P))
    return np.ascontiguousarray(P[p]), np.ascontiguousarray(M[p])


def variants():
    for nh, mp, nrm, ref in itertools.product((256, 1024), (1, 4), (False, True), (False, True)):
        yield "h%d_p%d%s%s" % (nh, mp, "_n" if nrm else "", "_r" if ref else ""), nh, mp, nrm, ref


def measure(reps, only):
    import torch
    from pcgol_amd import build as B
    from pcgol_amd import kdtree
    sync = torch.cuda.synchronize
    P, M = scene()
    n = len(P)
    t = kdtree.New(P)
    dev = "cuda"
    i32 = torch.int32
    d_nrm = torch.from_numpy(M).to(dev)
    smp = torch.from_numpy(np.random.default_rng(1).integers(0, 2 ** 32, 3 * 1024 * 4, dtype=np.uint64).astype(np.uint32)
                           .view(np.int32)).to(dev)
    d_n, d_sz, d_rf, d_bs = (torch.zeros(k, dtype=i32, device=dev) for k in (1, 4, 4, 4))
    d_pl = torch.zeros((4, 4), dtype=torch.float32, device=dev)
    d_lab, d_ids = (torch.zeros(n, dtype=i32, device=dev) for _ in range(2))

    def call(nh, mp, nrm, ref):
        def run():
            t.PlanesDev(MAX_DIST, smp.data_ptr(), nh, d_n.data_ptr(), d_pl.data_ptr(), d_sz.data_ptr(), d_rf.data_ptr(),
                        d_bs.data_ptr(), d_lab.data_ptr(), d_ids=d_ids.data_ptr(), MaxPlanes=mp, MinInliers=MIN_INLIERS,
                        d_normals=d_nrm.data_ptr() if nrm else 0, MinNormalCos=0.8, Refine=ref)
        return run

    calls = {k: call(*a) for k, *a in variants() if not only or k == only}
    out = {"points": n, "max_dist": MAX_DIST, "min_inliers": MIN_INLIERS, "reps": reps}
    ts = {k: [] for k in calls}
    for rep in range(reps + 2):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            sync()
            if rep >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3)
            if rep == 0:
                out[k + "_found"] = {"n_planes": int(d_n.item()), "sizes": d_sz.cpu().tolist(), "refined": d_rf.cpu().tolist()}
    for k, v in ts.items():
        out[k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
    print(json.dumps(out), flush=True)
    return {"source_hash": B.source_hash(), "calls": out}


def trace_summary(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    by = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0]
        if not any(k in name for k in ("planes_", "peel_", "gs_")):  # (peel_: consensus_peel.h's rounds)
            continue
        by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/planes_probe.py --reps 3 --only NAME "
                  "(no counters in the run); durations from the trace by kernel name, warm-up launches included",
           "kernels": {}}
    for name, v in sorted(by.items()):
        out["kernels"][name] = {"launches": len(v), "total_us": round(float(np.sum(v)), 1),
                                "median_us": round(float(np.median(v)), 2), "max_us": round(float(np.max(v)), 2)}
        if "planes_count_kernel" in name:
            out["kernels"][name]["busy_us"] = [round(x, 1) for x in v if x > 20.0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--only", default=None)
    ap.add_argument("--trace-summary", default=None)
    a = ap.parse_args()
    if a.trace_summary:
        res = {}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        res.setdefault("kernel_trace", {})[a.only or "all"] = trace_summary(a.trace_summary)
    else:
        res = measure(a.reps, a.only)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
