"""GPU probe: k-NN covariances (pcgx_kdtree_covariances_dev, csrc/knearest.hip in covariance mode) against
pcgx_kdtree_knearest_dev at the same k on the same queries -- the yardstick: the same search, with ids and DistSq
written instead of each list's points fetched, summed and solved.

    python tools/covariances_probe.py [--out profiles/covariances_probe.json] [--reps 21]

Case: the 1M-point synth.surface_cloud of width 30 (C4's plane scene), q == NULL, k = 20, on the grid and on the
forced tree walk (PCGX_RANGE_WALK=1).  Timed: knearest_dev; covariances_dev in PLANE mode with normals and counts;
in RAW mode without normals (no eigen-solve).  Each figure is the median of --reps calls after two warm-up calls, host
clock around the call and a device synchronise.
"""
import argparse
import ctypes as C
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


def case(base, k, reps, walk=False):
    import torch
    from pcgol_amd import _lib as L
    from pcgol_amd import kdtree
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    if walk:
        os.environ["PCGX_RANGE_WALK"] = "1"
    try:
        t = kdtree.New(base)
        lib = L.lib()
        n = len(base)
        di = torch.empty((n, k), dtype=torch.int32, device=dev)
        dd = torch.empty((n, k), dtype=torch.float32, device=dev)
        dc = torch.empty((n, 6), dtype=torch.float32, device=dev)
        dn = torch.empty((n, 3), dtype=torch.float32, device=dev)
        dk = torch.empty(n, dtype=torch.int32, device=dev)
        inf = float("inf")

        def knearest():
            L.check(lib.pcgx_kdtree_knearest_dev(t._h, None, n, k, inf, C.c_void_p(di.data_ptr()),
                                                 C.c_void_p(dd.data_ptr()), None, None))

        def plane():
            L.check(lib.pcgx_kdtree_covariances_dev(t._h, None, n, k, inf, L.PCGX_COV_PLANE, 1e-3, None,
                                                    C.c_void_p(dc.data_ptr()), C.c_void_p(dn.data_ptr()),
                                                    C.c_void_p(dk.data_ptr()), None))

        def raw():
            L.check(lib.pcgx_kdtree_covariances_dev(t._h, None, n, k, inf, L.PCGX_COV_RAW, 1e-3, None,
                                                    C.c_void_p(dc.data_ptr()), None, None, None))

        out = {"points": n, "k": k, "walk_forced": walk, "knearest_dev": timed(knearest, reps, sync),
               "covariances_dev_plane": timed(plane, reps, sync), "covariances_dev_raw": timed(raw, reps, sync)}
        kn = out["knearest_dev"]["median_ms"]
        out["plane_over_knearest"] = out["covariances_dev_plane"]["median_ms"] / kn
        out["raw_over_knearest"] = out["covariances_dev_raw"]["median_ms"] / kn
        print(json.dumps(out), flush=True)
        return out
    finally:
        os.environ.pop("PCGX_RANGE_WALK", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    from pcgol_amd import build as B
    from pcgol_amd import synth
    surf = synth.surface_cloud(1_000_000, 30.0, 6)[0]
    res = {"source_hash": B.source_hash(), "cases": {"surface_1M_own_k20": case(surf, 20, a.reps),
                                                     "surface_1M_own_k20_walk": case(surf, 20, a.reps, walk=True)}}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
