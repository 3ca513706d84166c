"""GPU probe: surface normals (pcgx_kdtree_normals_dev, csrc/normals.hip) against pcgx_kdtree_range_count on the
same queries -- the yardstick: it enumerates the same neighbour sets the same way, without the moments and the solve.

    python tools/normals_probe.py [--out profiles/normals_probe.json] [--reps 21]

Cases: (a) the 1M-point synth.surface_cloud of width 30 (C4's plane scene), q == NULL (the tree's own points),
r = 0.1, ~34 neighbours each; (b) 200k random queries in a 200k-point unit-cube cloud, r = 0.05, ~100 neighbours.
Each figure is the median of --reps timed calls after two warm-up calls, host clock around the call and a device
synchronise.  normals_dev is device resident (queries, outputs in HBM); range_count is the host entry point (it
uploads the queries and downloads int64 counts), so its figure includes those copies -- they are listed apart
(upload + download of the same byte counts, timed with torch) to give the kernel-side comparison.
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
from pcgol_amd import _lib as L  # noqa: E402
from pcgol_amd import build as B  # noqa: E402
from pcgol_amd import kdtree, synth  # noqa: E402


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


def case(name, base, queries, r, reps):
    import torch
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    t = kdtree.New(base)
    own = queries is None
    q = base if own else queries
    nq = len(q)
    dq = None if own else torch.from_numpy(q).to(dev)
    dn = torch.empty((nq, 3), dtype=torch.float32, device=dev)
    dc = torch.empty(nq, dtype=torch.float32, device=dev)
    dk = torch.empty(nq, dtype=torch.int32, device=dev)
    sync()
    lib = L.lib()
    vp = np.zeros(3, np.float32)

    def normals():
        L.check(lib.pcgx_kdtree_normals_dev(t._h, None if own else C.c_void_p(dq.data_ptr()), nq, r, L.ptr(vp), 3,
                                            C.c_void_p(dn.data_ptr()), C.c_void_p(dc.data_ptr()),
                                            C.c_void_p(dk.data_ptr()), None))

    counts = np.zeros(nq, np.int64)
    qh = np.ascontiguousarray(q, dtype=np.float32)

    def range_count():
        L.check(lib.pcgx_kdtree_range_count(t._h, L.ptr(qh), nq, r, L.ptr(counts)))

    hq = torch.from_numpy(qh.copy())
    hc = torch.from_numpy(np.empty_like(counts))
    dq2 = torch.empty_like(hq, device=dev)
    dc2 = torch.empty_like(hc, device=dev)

    def copies():  # what range_count moves over the bus besides its kernel
        dq2.copy_(hq)
        hc.copy_(dc2)

    out = {"points": len(base), "queries": nq, "own_points": own, "radius": r,
           "normals_dev": timed(normals, reps, sync), "range_count": timed(range_count, reps, sync),
           "range_count_copies": timed(copies, reps, sync)}
    k = dk.cpu().numpy()
    out["mean_neighbours"] = float(k.mean())
    out["counts_equal_range_count"] = bool(np.array_equal(k, counts))
    out["degenerate"] = int(np.isnan(dc.cpu().numpy()).sum())
    kern = out["range_count"]["median_ms"] - out["range_count_copies"]["median_ms"]
    out["range_count_minus_copies_ms"] = kern
    out["normals_over_range_count_kernel"] = out["normals_dev"]["median_ms"] / kern if kern > 0 else None
    print(name, json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    res = {"source_hash": B.source_hash(), "cases": {}}
    res["cases"]["surface_1M_own_r0.1"] = case("surface", synth.surface_cloud(1_000_000, 30.0, 6)[0], None, 0.1, a.reps)
    res["cases"]["cube_200k_queries_r0.05"] = case("cube", synth.uniform_cloud(200_000, 1.0, 11),
                                                   synth.uniform_cloud(200_000, 1.0, 14), 0.05, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
