"""GPU probe: statistical outlier removal (pcgx_sor_filter_dev, csrc/sor.hip) on the 1M-point synth.surface_cloud of
width 30 (C4's plane scene) with mean_k = 16, std_mul = 1, split into the tree build (pcgx_kdtree_build over the same
points, which the filter runs inside) and the rest.

    python tools/sor_probe.py [--out profiles/sor_probe.json] [--reps 11]

Each figure is the median of --reps timed calls after two warm-up calls, host clock around the call (the filter
returns when its stream is done; the build synchronises itself).  The records are device resident; "rest" is the
filter's median minus the build's: the finite-point compaction and the copy of the packed points to the host that the
build takes, the k-NN pass, the statistics and the output compaction.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    import torch
    from pcgol_amd import _lib as L
    from pcgol_amd import build as B
    from pcgol_amd import outlier, synth
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    pts = synth.surface_cloud(1_000_000, 30.0, 6)[0]
    n = len(pts)
    lib = L.lib()
    d_in = torch.from_numpy(pts.copy()).to(dev)
    d_out = torch.empty_like(d_in)
    d_md = torch.empty(n, dtype=torch.float64, device=dev)
    f = outlier.New(16, 1.0)
    kept = [0]

    def sor():
        kept[0] = f.FilterDev(d_in.data_ptr(), n, 12, 0, d_out.data_ptr(), d_md.data_ptr())

    def build():
        h = C.c_void_p()
        L.check(lib.pcgx_kdtree_build(L.ptr(pts), n, 12, 0, C.byref(h)))
        L.check(lib.pcgx_kdtree_free(h))

    res = {"source_hash": B.source_hash(), "points": n, "mean_k": 16, "std_mul": 1.0,
           "sor_filter_dev": timed(sor, a.reps, sync), "tree_build": timed(build, a.reps, sync)}
    res["kept"] = kept[0]
    res["stats_mu_sigma_T"] = list(f.Stats)
    res["rest_ms"] = res["sor_filter_dev"]["median_ms"] - res["tree_build"]["median_ms"]
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
