"""GPU probe: consistent normal orientation (pcgx_kdtree_orient_normals_dev; csrc/orient.hip) against its yardsticks,
all taken in the same run.

    python tools/orient_probe.py [--out profiles/orient_probe.json] [--reps 11] [--points 1000000]

Cases: synth.surface_cloud(1_000_000, 30, 6) (about 1100 points per square metre, spacing 0.03) at r = 0.1 (~35
neighbours) and at r = 0.03, the point spacing (~3 neighbours); the normals are NormalsDev's with every sign randomised.
Per case:
  orient_dev             OrientNormalsDev in its three modes with max_rounds = 0 (enough rounds to finish for certain), and
                         in mode 0 with exactly the rounds it needs;
  rounds                 the points in the active list before each round (the probe entry point's d_active), and how many
                         rounds had any;
  normals_dev            yardstick: ONE enumeration of the same neighbourhoods;
  clusters_dev           yardstick: TWO enumerations and a union-find over the same graph (oriented, min_cos 0).
active_list says whether the library was built with the active list (PCGX_EXTRA_CFLAGS=-DPCGX_ORIENT_ACTIVE_LIST=0 builds
it without: run the probe on both builds, alternately, to see what the list buys).
Each figure is the median of --reps timed calls after two warm-up calls, host clock around the call and a device
synchronise."""
import argparse
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


def case(pts, r, reps):
    import torch
    from pcgol_amd import _lib as L
    from pcgol_amd import kdtree
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    t = kdtree.New(pts)
    n = len(pts)
    full = int(L.lib().pcgx_orient_full_rounds(n))
    dn = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dcurv = torch.empty(n, dtype=torch.float32, device=dev)
    do = torch.empty((n, 3), dtype=torch.float32, device=dev)
    df = torch.empty(n, dtype=torch.uint8, device=dev)
    di = torch.empty(n, dtype=torch.int32, device=dev)
    dc = torch.zeros(2, dtype=torch.int32, device=dev)
    dact = torch.zeros(full + 1, dtype=torch.int32, device=dev)
    sync()
    t.NormalsDev(r, dn.data_ptr(), dcurv.data_ptr())
    sign = torch.from_numpy(np.where(np.random.default_rng(5).integers(0, 2, n) == 1, -1.0, 1.0).astype(np.float32)).to(dev)
    dn *= sign[:, None]
    sync()
    up = np.array([0, 0, 1], np.float32)
    eye = np.array([0, 0, 50], np.float32)

    def orient(mode, ref, rounds):
        t.OrientNormalsDev(r, dn.data_ptr(), do.data_ptr(), df.data_ptr(), dc.data_ptr(), dc.data_ptr() + 4,
                           Direction=ref if mode == 1 else None, Viewpoint=ref if mode == 2 else None, MaxRounds=rounds)

    L.check(L.lib().pcgx_kdtree_orient_normals_probe_dev(t._h, float(r), L.ptr(dn.data_ptr()), 0, None, 0, L.ptr(do.data_ptr()),
                                                         L.ptr(df.data_ptr()), L.ptr(dc.data_ptr()), L.ptr(dc.data_ptr() + 4),
                                                         L.ptr(dact.data_ptr()), None))
    sync()
    active = [int(v) for v in dact.cpu().numpy()]
    counts = dc.cpu().numpy()
    needed = sum(1 for v in active[:-1] if v > 0)
    out = {"points": n, "radius": r, "full_rounds": full, "rounds_needed": needed, "active_before_round": active,
           "components": int(counts[0]), "open": int(counts[1]), "flipped": int(df.sum().item())}
    out["orient_dev"] = {"mode0": timed(lambda: orient(0, None, 0), reps, sync),
                         "mode1_direction": timed(lambda: orient(1, up, 0), reps, sync),
                         "mode2_viewpoint": timed(lambda: orient(2, eye, 0), reps, sync),
                         "mode0_exact_rounds": timed(lambda: orient(0, None, max(needed, 1)), reps, sync)}
    out["normals_dev"] = timed(lambda: t.NormalsDev(r, do.data_ptr(), dcurv.data_ptr()), reps, sync)
    out["clusters_dev"] = timed(lambda: t.ClustersDev(r, di.data_ptr(), dc.data_ptr(), d_normals=dn.data_ptr(), MinCos=0.0,
                                                      Oriented=True), reps, sync)
    m = out["orient_dev"]["mode0"]["median_ms"]
    out["ratio_to_normals_dev"] = m / out["normals_dev"]["median_ms"]
    out["ratio_to_clusters_dev"] = m / out["clusters_dev"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_probe.json"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--points", type=int, default=1_000_000)
    a = ap.parse_args()
    from pcgol_amd import _lib as L
    from pcgol_amd import build, synth
    pts = synth.surface_cloud(a.points, 30, 6)[0]
    res = {"tool": "tools/orient_probe.py", "source_hash": build.source_hash(),
           "active_list": int(L.lib().pcgx_orient_active_list()),
           "cases": {"r0.1": case(pts, 0.1, a.reps), "r0.03": case(pts, 0.03, a.reps)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
