"""GPU probe: sample consensus plane detection (pcgol_amd.sac, csrc/sac.hip) on the large scene of
tests/test_gpu_sac.py::test_scale_global_bits -- 1.55M points, a 256 x 256 x 128 grid (8.4M voxels) at 0.04 with
more occupied voxels than the LDS bitmap holds (the global-bits path).

    python tools/sac_probe.py [--out profiles/sac_probe.json] [--reps 5]

Times, with a host clock around each call (every call ends in a device synchronise): model creation, Compute(n) for
n in {30, 256, 1024, 4096} (the 3n ids drawn by a seeded sampler before the clock starts), Inliers(0.05) of the
chosen plane, and the small scene of the reference's TestSAC (Compute(30)).  The CPU figure is the NumPy oracle's
(tests/sac_oracle.py, one core, vectorised lattice) for the n = 30 hypotheses: not Go's.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pcgol_amd import build as B  # noqa: E402
from pcgol_amd import sac, segmentation  # noqa: E402


def large_scene():
    rng = np.random.default_rng(11)
    res, size = 0.04, (256, 256, 128)
    origin = np.array([-5.0, -4.0, -0.5], np.float32)
    e = np.array(size) * res
    floor = np.c_[rng.random(400000) * e[0], rng.random(400000) * e[1], 0.3 + rng.normal(0, 0.004, 400000)]
    wall = np.c_[rng.random(250000) * e[0], 2.5 + rng.normal(0, 0.004, 250000), rng.random(250000) * e[2]]
    ramp_xy = rng.random((150000, 2)) * e[:2]
    ramp = np.c_[ramp_xy, 0.4 * ramp_xy[:, 0] + rng.normal(0, 0.004, 150000)]
    clutter = rng.random((750000, 3)) * e
    pts = (np.concatenate([floor, wall, ramp, clutter]) + origin).astype(np.float32)
    return res, size, origin, pts


def timed(fn, reps):
    fn()  # warm-up (code objects, arena growth)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    res, size, origin, pts = large_scene()
    g = segmentation.StorageVoxelGrid(res, size, origin)
    g.AddAll(pts)
    n_len, n_added, n_occ = g._counts()
    rec = {"source_hash": B.source_hash(), "scene": {"points": len(pts), "voxels": n_len, "added": n_added,
                                                    "occupied": n_occ, "resolution": res, "size": list(size)}}
    m, rec["model_create"] = timed(lambda: sac.NewVoxelGridSurfaceModel(g, pts), a.reps)
    rec["compute"] = {}
    best = None
    for n in (30, 256, 1024, 4096):
        smp = sac.NewRandomSampler(len(pts), n)
        ids = np.array([smp.Sample() for _ in range(3 * n)], np.int64)
        r, t = timed(lambda: m.compute(ids, per_hypothesis=False), a.reps)
        _, _, _, _, ok, _, score = m.compute(ids)
        t.update({"found": r[0], "best": r[1], "best_score": r[2], "ok": int(ok.sum()), "mean_score": float(score.mean())})
        rec["compute"][str(n)] = t
        print("Compute(%4d): %8.3f ms median (%.3f-%.3f), %d ok, best %d score %d" %
              (n, t["median_ms"], t["min_ms"], t["max_ms"], t["ok"], r[1], r[2]), flush=True)
        if n == 30:
            best, ids30 = r[3], ids
    inl, rec["inliers_0.05"] = timed(lambda: best.Inliers(0.05), a.reps)
    rec["inliers_0.05"]["count"] = int(len(inl))
    print("Inliers(0.05): %.3f ms median, %d ids" % (rec["inliers_0.05"]["median_ms"], len(inl)))
    # the reference's TestSAC scene (13 points, 8^3 grid): what one Compute(30) costs at toy size
    small = np.array([[0, 0, 0], [0.1, 0, 0.1], [0.2, 0, 0.2], [0.2, 0.1, 0.6], [0, 0.1, 0], [0.1, 0.1, 0.1],
                      [0.2, 0.1, 0.2], [0, 0.2, 0], [0.1, 0.2, 0.1], [0.2, 0.2, 0.2], [0.3, -0.1, 0], [0.6, 0.7, 0],
                      [0.6, 0.3, 0]], np.float32)
    sg = segmentation.StorageVoxelGrid(0.1, (8, 8, 8), (0, 0, 0))
    sg.AddAll(small)
    sm = sac.NewVoxelGridSurfaceModel(sg, small)
    sids = np.random.default_rng(0).integers(0, len(small), size=90)
    _, rec["small_compute_30"] = timed(lambda: sm.compute(sids, per_hypothesis=False), max(a.reps, 20))
    print("TestSAC scene Compute(30): %.3f ms median" % rec["small_compute_30"]["median_ms"])
    if not a.no_oracle:
        import sac_oracle as S
        om = S.SurfaceModel(S.Grid(res, size, origin, pts), pts)
        t0 = time.perf_counter()
        o = S.compute(om, ids30, 30)
        rec["numpy_oracle_compute_30_ms"] = (time.perf_counter() - t0) * 1e3
        rec["numpy_oracle_agrees"] = (o[0], o[1], o[2]) == tuple(rec["compute"]["30"][k] for k in ("found", "best", "best_score"))
        print("NumPy oracle (one CPU core, not Go) Compute(30): %.1f ms, agrees: %s" %
              (rec["numpy_oracle_compute_30_ms"], rec["numpy_oracle_agrees"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
