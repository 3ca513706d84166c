"""GPU probe: cylinder and sphere segmentation (csrc/shapes.hip) -- ShapesDev on a 1M-point scene: one upright cylinder
from 1024 hypotheses, four cylinders from 256 hypotheses each (refined and not), one sphere, and the yardstick: PlanesDev
with normals on the same cloud at the same hypothesis counts.

    python tools/shapes_probe.py [--out profiles/shapes_probe.json] [--reps 11] [--only NAME]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/shapes_probe.py --reps 3 --only NAME
    python tools/shapes_probe.py --trace-summary DIR --only NAME --out profiles/shapes_probe.json  (adds "kernel_trace")

Workload: the base of synth.c4_plane(600_000) (a gently waved ground, 23 m wide) with its normals, four upright poles of
75 000 points each (radii 0.4 .. 0.7, 6 m high, radial noise 0.01), a ball of 50 000 (radius 1) and 50 000 clutter points
with random normals, shuffled; every normal perturbed by N(0, 0.05) a component and renormalised.  max_dist 0.05,
min_inliers 30 000, min_normal_cos 0.8, sample_radius 0.8, r in [0.2, 1.5].  The calls alternate in one process; each
repetition times every call in turn (host clock around the call and a device synchronise, the method of
tools/planes_probe.py) after two warm-up rounds; the figures are medians over --reps rounds with min and max.  The trace
summary sums the kernels of a run by name (run it with --only: one kind of call in the trace)."""
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

MAX_DIST, MIN_INLIERS, MIN_COS, SAMPLE_RADIUS, R_MIN, R_MAX = 0.05, 30_000, 0.8, 0.8, 0.2, 1.5
POLES = ((5.0, 5.0, 0.4), (17.0, 6.0, 0.5), (8.0, 16.0, 0.6), (16.0, 17.0, 0.7))
BALL = (11.0, 11.0, 4.0, 1.0)


def scene():
    from pcgol_amd import synth
    c = synth.c4_plane(600_000)
    rng = np.random.default_rng(23)
    w = 30.0 * 0.6 ** 0.5
    P, M = [c["base"]], [c["normals"]]
    for x, y, r in POLES:
        phi, z = rng.random(75_000) * 2 * np.pi, rng.random(75_000) * 6
        d = np.column_stack([np.cos(phi), np.sin(phi), np.zeros(75_000)])
        P.append(np.array([x, y, 0.0]) + d * (r + rng.normal(0, 0.01, 75_000))[:, None] + z[:, None] * (0, 0, 1))
        M.append(d)
    d = rng.standard_normal((50_000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    P.append(np.array(BALL[:3]) + d * (BALL[3] + rng.normal(0, 0.01, 50_000))[:, None])
    M.append(d)
    r = rng.standard_normal((50_000, 3))
    P.append(rng.random((50_000, 3)) * (w, w, 7))
    M.append(r / np.linalg.norm(r, axis=1)[:, None])
    P, M = np.concatenate(P), np.concatenate(M)
    M = M + rng.normal(0, 0.05, M.shape)
    M /= np.linalg.norm(M, axis=1)[:, None]
    p = rng.permutation(len(P))
    return np.ascontiguousarray(P[p], np.float32), np.ascontiguousarray(M[p], np.float32)


# name -> (what, n_hyp, rounds, refine, upright)
VARIANTS = {
    "cyl_h1024_s1": ("cylinder", 1024, 1, False, True),
    "cyl_h256_s4": ("cylinder", 256, 4, False, False),
    "cyl_h256_s4_r": ("cylinder", 256, 4, True, False),
    "sph_h1024_s1": ("sphere", 1024, 1, False, False),
    "planes_h1024_p1_n": ("plane", 1024, 1, False, False),
    "planes_h256_p4_n_r": ("plane", 256, 4, True, False),
}


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
    d_sh = torch.zeros((4, 8), dtype=torch.float32, device=dev)
    d_lab, d_ids = (torch.zeros(n, dtype=i32, device=dev) for _ in range(2))

    def call(what, nh, rounds, refine, upright):
        def shapes():
            t.ShapesDev(1 if what == "cylinder" else 0, MAX_DIST, d_nrm.data_ptr(), smp.data_ptr(), nh, d_n.data_ptr(),
                        d_sh.data_ptr(), d_sz.data_ptr(), d_rf.data_ptr(), d_bs.data_ptr(), d_lab.data_ptr(),
                        d_ids=d_ids.data_ptr(), MaxShapes=rounds, MinInliers=MIN_INLIERS, SampleRadius=SAMPLE_RADIUS, RMin=R_MIN,
                        RMax=R_MAX, Axis=(0, 0, 1) if upright else None, MinAxisCos=0.95, MinNormalCos=MIN_COS, Refine=refine)

        def planes():
            t.PlanesDev(0.25, smp.data_ptr(), nh, d_n.data_ptr(), d_sh.data_ptr(), d_sz.data_ptr(), d_rf.data_ptr(),
                        d_bs.data_ptr(), d_lab.data_ptr(), d_ids=d_ids.data_ptr(), MaxPlanes=rounds, MinInliers=MIN_INLIERS,
                        d_normals=d_nrm.data_ptr(), MinNormalCos=MIN_COS, Refine=refine)
        return planes if what == "plane" else shapes

    calls = {k: call(*a) for k, a in VARIANTS.items() if not only or k == only}
    out = {"points": n, "max_dist": MAX_DIST, "min_inliers": MIN_INLIERS, "min_normal_cos": MIN_COS,
           "sample_radius": SAMPLE_RADIUS, "r_min": R_MIN, "r_max": R_MAX, "reps": reps}
    ts = {k: [] for k in calls}
    for rep in range(reps + 2):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            sync()
            if rep >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3)
            if rep == 0:
                out[k + "_found"] = {"n": int(d_n.item()), "sizes": d_sz.cpu().tolist(), "refined": d_rf.cpu().tolist(),
                                     "records": d_sh.cpu().numpy().round(4).tolist()}
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
        if not any(k in name for k in ("shapes_", "planes_", "peel_", "gs_")):  # (peel_: consensus_peel.h's rounds)
            continue
        by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/shapes_probe.py --reps 3 --only NAME "
                  "(no counters in the run); durations from the trace by kernel name, warm-up launches included",
           "kernels": {}}
    for name, v in sorted(by.items()):
        out["kernels"][name] = {"launches": len(v), "total_us": round(float(np.sum(v)), 1),
                                "median_us": round(float(np.median(v)), 2), "max_us": round(float(np.max(v)), 2)}
        if "count_kernel" in name or "partner_kernel" in name:
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
