"""GPU probe: ray queries (csrc/rays.hip) -- RayCastDev and RayPierceDev on a 1M-point surface cloud with 100 000
LiDAR-like rays and a radius near the point spacing, beside what a user could do without them.

    python tools/rays_probe.py [--out profiles/rays_probe.json] [--reps 11] [--batch 5]

One process, one GPU.  A call time is a host clock around --batch calls in a row and one device synchronise, divided by
the batch; a kernel time is a pair of events round one call on the stream (each call is one launch).  Two warm-up rounds,
then medians over --reps rounds; "spread_ms" (max - min) is what a difference has to exceed.
  raycast / pierce            RayCastDev with every output / RayPierceDev, on the grid
  raycast_walk / pierce_walk  ... under PCGX_RANGE_WALK=1
  slabs                       slabs per ray as the kernel cuts them (the clip and the slab count restated in NumPy)
  candidates                  on a sample of rays: records the balls of a ray's slabs report (pcgx_kdtree_range_count at
                              the slab centres with the ray's bound), against the members among them
  range_batch                 the same sample answered by RangeBatch at points along the rays, 2 rho apart, and the member
                              test in torch: what a user can do today
  brute_force                 the same sample against all points in torch float64, in chunks"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_POINTS, WIDTH, RHO = 1_000_000, 30.0, 0.03  # the points' spacing is 30 / sqrt(1M) = 0.03
SENSOR = (15.0, 15.0, 4.0)
SAMPLE = 1000
U = 2.0 ** -20


def clip_and_slabs(o, d, rho, lo, hi, target):
    """ray_clip and ray_slabs of csrc/ray_terms.h for rays with s in [0, +inf), vectorised: (ok, a0, a1, K)"""
    o, d, rho = o.astype(np.float64), d.astype(np.float64), float(np.float32(rho))
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    mag = np.maximum(np.abs(o).max(1), max(np.abs(lo).max(), np.abs(hi).max()))
    pad = (rho * (1.0 + U) + U * mag)[:, None]
    with np.errstate(all="ignore"):
        t0, t1 = (lo[None, :] - pad - o) / d, (hi[None, :] + pad - o) / d
        par = d == 0.0
        out = (par & ((o < lo[None, :] - pad) | (o > hi[None, :] + pad))).any(1)
        s0 = np.where(par, -np.inf, np.minimum(t0, t1)).max(1)
        s1 = np.where(par, np.inf, np.maximum(t0, t1)).min(1)
    a0, a1 = np.maximum(s0 * dd, 0.0), s1 * dd
    ok = ~out & (a0 <= a1)
    q = np.where(ok, (a1 - a0) / np.sqrt(dd) / target, 0.0)
    K = np.where(ok, np.where(q >= 4095, 4096, q.astype(np.int64) + 1), 0)
    return ok, a0, a1, K, dd, mag


def measure(reps, batch):
    import torch
    from pcgol_amd import _lib as L
    from pcgol_amd import build as B
    from pcgol_amd import kdtree, rays, synth
    sync = torch.cuda.synchronize
    P = synth.surface_cloud(N_POINTS, WIDTH, 6)[0]
    n = len(P)
    t = kdtree.New(P)
    geom, dims = np.zeros(5, np.float32), np.zeros(3, np.int32)
    L.check(L.lib().pcgx_debug_grid_geometry(t._h, L.ptr(geom), L.ptr(dims)))
    h = float(geom[3])
    # a spinning sensor above the surface: 1000 azimuths x 100 beams looking down between 3 and 60 degrees
    o, d = rays.spherical_rays(SENSOR, np.linspace(-np.pi, np.pi, 1000, endpoint=False), np.radians(np.linspace(-60, -3, 100)))
    nr = len(o)
    dev = "cuda"
    d_o, d_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    d_ids = torch.zeros(nr, dtype=torch.int32, device=dev)
    d_along, d_off = (torch.zeros(nr, dtype=torch.float64, device=dev) for _ in range(2))
    d_counts = torch.zeros(n, dtype=torch.int32, device=dev)

    def walk(fn):
        def run():
            os.environ["PCGX_RANGE_WALK"] = "1"  # (read per call)
            fn()
            os.environ.pop("PCGX_RANGE_WALK", None)
        return run

    stream = torch.cuda.Stream()  # the calls and the events that time them go on one stream
    st = stream.cuda_stream

    def raycast():
        t.RayCastDev(d_o.data_ptr(), d_d.data_ptr(), nr, RHO, d_ids.data_ptr(), d_along.data_ptr(), d_off.data_ptr(), stream=st)

    def pierce():
        t.RayPierceDev(d_o.data_ptr(), d_d.data_ptr(), nr, RHO, d_counts.data_ptr(), stream=st)

    calls = {"raycast": raycast, "pierce": pierce, "raycast_walk": walk(raycast), "pierce_walk": walk(pierce)}
    out = {"points": n, "rays": nr, "radius": RHO, "grid_cell": h, "reps": reps, "batch": batch}
    ts, ks = {k: [] for k in calls}, {k: [] for k in calls}
    for rep in range(reps + 2):
        for k, fn in calls.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(batch):
                fn()
            sync()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            sync()
            if rep >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3 / (batch + 1))
                ks[k].append(e0.elapsed_time(e1))
    for k in calls:
        out[k] = {"median_ms": float(np.median(ts[k])), "min_ms": float(np.min(ts[k])), "max_ms": float(np.max(ts[k])),
                  "spread_ms": float(np.max(ts[k]) - np.min(ts[k])), "kernel_median_ms": float(np.median(ks[k])),
                  "kernel_min_ms": float(np.min(ks[k]))}
    ids = d_ids.cpu().numpy()
    d_counts.zero_()
    pierce()
    sync()
    counts = d_counts.cpu().numpy()
    out["hits"] = int((ids >= 0).sum())
    out["members"] = int(counts.sum())
    # ---- slabs per ray
    lo, hi = P.min(0).astype(np.float64), P.max(0).astype(np.float64)
    for name, target in (("grid", max(2 * RHO, h)), ("walk", 2 * RHO)):
        ok, a0, a1, K, dd, mag = clip_and_slabs(o, d, RHO, lo, hi, target)
        out["slabs_" + name] = {"mean": float(K.mean()), "median": float(np.median(K)), "max": int(K.max()),
                                "rays_clipped_away": int((~ok).sum()), "rounds_of_64_mean": float(np.ceil(K / 64).mean())}
    # ---- candidates per member, on a sample of rays (the grid's slabs)
    ok, a0, a1, K, dd, mag = clip_and_slabs(o, d, RHO, lo, hi, max(2 * RHO, h))
    rng = np.random.default_rng(3)
    sample = np.sort(rng.choice(np.nonzero(ok)[0], SAMPLE, replace=False))
    cand = 0
    for i in sample:
        k = np.arange(K[i])
        b0 = np.minimum(a0[i] + (a1[i] - a0[i]) * (k / K[i]), a1[i])
        b1 = np.append(b0[1:], a1[i])
        s = 0.5 * (b0 + b1) / dd[i]
        c = np.clip(o[i].astype(np.float64) + s[:, None] * d[i].astype(np.float64), lo, hi).astype(np.float32)
        um = U * mag[i]
        half = 0.5 * (a1[i] - a0[i]) / K[i] / np.sqrt(dd[i])
        R = np.sqrt((RHO * (1 + U) + um) ** 2 + (half * (1 + U) + um) ** 2) + um
        bound = np.float32(R * R * (1 + 2.0 ** -18) * (1 + U))
        cnt = np.zeros(len(c), np.int64)
        L.check(L.lib().pcgx_kdtree_range_count(t._h, L.ptr(np.ascontiguousarray(c)), len(c), float(np.sqrt(np.float64(bound))),
                                                L.ptr(cnt)))
        cand += int(cnt.sum())
    so, sd = np.ascontiguousarray(o[sample]), np.ascontiguousarray(d[sample])
    members = int(t.RayPierce(so, sd, RHO).sum())
    out["candidates"] = {"sample_rays": SAMPLE, "candidates": cand, "members": members,
                         "candidates_per_member": cand / max(members, 1),
                         "note": "range_count at the slab centres with radius sqrt(bound): within a rounding of the kernel's set"}
    # ---- the same sample by RangeBatch along the rays and the member test in torch
    want = t.RayCast(so, sd, RHO)

    def member_first(po, pd, cand_pts, cand_ids, owner):
        """first hits of rays (po, pd) among candidate points owned by ray `owner`, in torch float64"""
        w = cand_pts.double() - po.double()[owner]
        dv = pd.double()[owner]
        a = (w[:, 0] * dv[:, 0] + w[:, 1] * dv[:, 1]) + w[:, 2] * dv[:, 2]
        c = torch.cross(w, dv, dim=1)
        cc = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        ddv = (dv * dv).sum(1)
        m = (cc <= (RHO * RHO) * ddv) & (a >= 0)
        key = torch.where(m, a, torch.full_like(a, float("inf")))
        best = torch.full((len(po),), float("inf"), dtype=torch.float64, device=po.device)
        best.scatter_reduce_(0, owner, key, "amin")
        win = m & (key == best[owner])
        first = torch.full((len(po),), 2 ** 62, dtype=torch.int64, device=po.device)
        first.scatter_reduce_(0, owner[win], cand_ids[win], "amin")
        return torch.where(first < 2 ** 62, first, torch.full_like(first, -1))

    def range_batch():
        step = 2 * RHO
        length = (a1[sample] - a0[sample]) / np.sqrt(dd[sample])
        m = np.ceil(length / step).astype(np.int64) + 1
        owner = np.repeat(np.arange(SAMPLE), m)
        k = np.arange(m.sum()) - np.repeat(np.cumsum(m) - m, m)
        s = (a0[sample] / dd[sample])[owner] + k * step / np.sqrt(dd[sample])[owner]
        q = (so[owner].astype(np.float64) + s[:, None] * sd[owner].astype(np.float64)).astype(np.float32)
        offs, nid, _ = t.RangeBatch(q, float(np.sqrt(RHO * RHO + 0.25 * step * step) * 1.001))
        cown = torch.from_numpy(np.repeat(owner, np.diff(offs))).to(dev)
        cid = torch.from_numpy(nid).to(dev)
        first = member_first(torch.from_numpy(so).to(dev), torch.from_numpy(sd).to(dev), d_P[cid], cid, cown)
        sync()
        return first.cpu().numpy(), len(q), len(nid)

    d_P = torch.from_numpy(P).to(dev)
    range_batch()
    t0 = time.perf_counter()
    got, nq, ncand = range_batch()
    rb = (time.perf_counter() - t0) * 1e3
    out["range_batch"] = {"sample_rays": SAMPLE, "ms": rb, "queries": nq, "candidates": ncand,
                          "same_first_hits": bool(np.array_equal(got, want[0]))}

    def brute():
        res = []
        po, pd = torch.from_numpy(so).to(dev), torch.from_numpy(sd).to(dev)
        ids_all = torch.arange(n, device=dev)
        for f in range(0, SAMPLE, 50):
            e = min(f + 50, SAMPLE)
            owner = torch.arange(e - f, device=dev).repeat_interleave(n)
            first = member_first(po[f:e], pd[f:e], d_P.repeat(e - f, 1), ids_all.repeat(e - f), owner)
            res.append(first)
        sync()
        return torch.cat(res).cpu().numpy()

    brute()
    t0 = time.perf_counter()
    got = brute()
    bf = (time.perf_counter() - t0) * 1e3
    out["brute_force"] = {"sample_rays": SAMPLE, "ms": bf, "same_first_hits": bool(np.array_equal(got, want[0]))}
    # the library on the same sample, device resident
    d_so, d_sd = torch.from_numpy(so).to(dev), torch.from_numpy(sd).to(dev)
    v = []
    for rep in range(reps + 2):
        sync()
        t0 = time.perf_counter()
        for _ in range(batch):
            t.RayCastDev(d_so.data_ptr(), d_sd.data_ptr(), SAMPLE, RHO, d_ids.data_ptr())
        sync()
        if rep >= 2:
            v.append((time.perf_counter() - t0) * 1e3 / batch)
    out["raycast_sample"] = {"sample_rays": SAMPLE, "median_ms": float(np.median(v))}
    out["ratio_range_batch"] = rb / float(np.median(v))
    out["ratio_brute_force"] = bf / float(np.median(v))
    print(json.dumps(out), flush=True)
    return {"source_hash": B.source_hash(), "calls": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--batch", type=int, default=5)
    a = ap.parse_args()
    res = measure(a.reps, a.batch)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
