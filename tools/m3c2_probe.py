"""GPU probe: cylinder statistics and M3C2 (csrc/m3c2.hip) -- two 1M-point surface clouds, epoch 2 perturbed, 100 000
cores from ThinDev with Normals' directions, radius 0.1 (several point spacings), half lengths 0.5 and 2.0 (and 1.4,
where 16 lanes per cylinder are admissible), device forms, beside the ray queries' enumeration and what a user could do
without the feature.

    python tools/m3c2_probe.py [--out profiles/m3c2_probe.json] [--reps 11] [--batch 5]

One process, one GPU.  A call time is a host clock around --batch calls in a row and one device synchronise, divided by
the batch; a kernel time is a pair of events round one call on the stream (a statistics call is one launch).  Two warm-up
rounds, then medians over --reps rounds, the variants alternated inside every round; "spread_ms" (max - min) is what a
difference has to exceed.  Per half length L:
  stats1 / stats2 / finish / chain   CylinderStatsDev against each epoch, the finish, and M3C2.ComputeDev (all three)
  lanes_8 / lanes_16 / lanes_64      stats1 under PCGX_CYL_LANES: every admissible number of lanes per cylinder
  walk                               stats1 under PCGX_RANGE_WALK=1
  pierce                             RayPierceDev on the same tubes (unit axes, s in [-L, L]): the same enumeration with an
                                     integer atomic in place of the sums
  range_batch                        on 1000 cores: RangeBatch at radius sqrt(rho^2 + L^2), the member test and the sums in
                                     torch float64 -- what a user can do today -- against stats1 on the same cores,
                                     both over the same warm-ups and rounds
Not measured: the split of a statistics launch into enumeration and arithmetic, the float64 share, counters."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_POINTS, WIDTH, RHO = 1_000_000, 30.0, 0.1  # the points' spacing is 30 / sqrt(1M) = 0.03
HALVES = (0.5, 1.4, 2.0)
N_CORES, THIN_RADIUS = 100_000, 0.07
SAMPLE = 1000


def admissible(half, target):
    """the numbers of lanes per cylinder pcgx_kdtree_cylinder_stats may take (csrc/m3c2_terms.h, cyl_slab_bound)"""
    kb = 2.0 * half * (1.0 + 2.0 ** -40) / target + 1.0
    return [w for w in (8, 16, 64) if w >= kb or w == 64]


def decide(by_half):
    """The rule for the narrow kernels: a number of lanes below 64 stays in the code only where it is not slower than 64
    lanes at every half length at which it was measured (medians, alternated in one run; a difference inside the two
    spreads counts as not slower)."""
    verdict = {}
    for w in (8, 16):
        seen = []
        for half, res in by_half.items():
            a, b = res.get("lanes_%d" % w), res.get("lanes_64")
            if a and b:
                seen.append({"half_length": half, "ms": a["median_ms"], "ms_64_lanes": b["median_ms"],
                             "not_slower": a["median_ms"] <= b["median_ms"] + a["spread_ms"] + b["spread_ms"]})
        verdict["lanes_%d" % w] = {"measured_at": seen, "kept": bool(seen) and all(s["not_slower"] for s in seen)}
    verdict["taken_out"] = [k for k, v in verdict.items() if not v["kept"]]
    return verdict


def measure(reps, batch):
    import torch
    from pcgol_amd import _lib as L
    from pcgol_amd import build as B
    from pcgol_amd import change, kdtree, synth
    sync = torch.cuda.synchronize
    dev = "cuda"
    rng = np.random.default_rng(1)
    P1 = synth.surface_cloud(N_POINTS, WIDTH, 6)[0]
    P2 = synth.surface_cloud(N_POINTS, WIDTH, 7)[0]
    P2[:, 2] += (0.05 * (P2[:, 0] > 0.5 * WIDTH) + rng.normal(scale=0.005, size=N_POINTS)).astype(np.float32)
    n = len(P1)
    t1, t2 = kdtree.New(P1), kdtree.New(P2)
    geom, dims = np.zeros(5, np.float32), np.zeros(3, np.int32)
    L.check(L.lib().pcgx_debug_grid_geometry(t1._h, L.ptr(geom), L.ptr(dims)))
    h = float(geom[3])
    target = max(2 * RHO, h)
    stream = torch.cuda.Stream()  # the calls and the events that time them go on one stream
    st = stream.cuda_stream
    # ---- cores and normals, device resident
    d_ids = torch.zeros(n, dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    d_nrm = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    t1.ThinDev(THIN_RADIUS, d_ids.data_ptr(), d_cnt[0:].data_ptr(), d_cnt[1:].data_ptr(), stream=st)
    t1.NormalsDev(0.15, d_nrm.data_ptr(), stream=st)
    sync()
    kept, left = (int(v) for v in d_cnt.cpu().numpy())
    m = min(kept, N_CORES)
    pick = d_ids[:m].long()
    d_P1 = torch.from_numpy(P1).to(dev)
    d_cores = d_P1[pick].contiguous()
    d_axes = d_nrm[pick].contiguous()
    d_unit = (d_axes / d_axes.norm(dim=1, keepdim=True).clamp_min(1e-30)).contiguous()
    d_n1, d_n2 = (torch.zeros(m, dtype=torch.int32, device=dev) for _ in range(2))
    d_s1, d_s2 = (torch.zeros(2 * m, dtype=torch.float64, device=dev) for _ in range(2))
    d_dist, d_lod = (torch.zeros(m, dtype=torch.float64, device=dev) for _ in range(2))
    d_sig = torch.zeros(m, dtype=torch.uint8, device=dev)
    d_pierced = torch.zeros(n, dtype=torch.int32, device=dev)
    out = {"points": n, "cores": m, "thin_kept": kept, "thin_left": left, "radius": RHO, "grid_cell": h,
           "slab_length": target, "reps": reps, "batch": batch, "by_half_length": {}}

    def env(name, value, fn):
        def run():
            os.environ[name] = value  # (read per call)
            fn()
            os.environ.pop(name, None)
        return run

    for half in HALVES:
        m3 = change.M3C2(RHO, half, change.WithRegistrationError(0.01))
        d_lo = torch.full((m,), -half, dtype=torch.float32, device=dev)
        d_hi = torch.full((m,), half, dtype=torch.float32, device=dev)

        def stats1():
            t1.CylinderStatsDev(d_cores.data_ptr(), d_axes.data_ptr(), m, RHO, half, d_n1.data_ptr(), d_s1.data_ptr(), st)

        def stats2():
            t2.CylinderStatsDev(d_cores.data_ptr(), d_axes.data_ptr(), m, RHO, half, d_n2.data_ptr(), d_s2.data_ptr(), st)

        def finish():
            L.check(L.lib().pcgx_m3c2_finish_dev(
                L.ptr(d_axes.data_ptr()), L.ptr(d_n1.data_ptr()), L.ptr(d_s1.data_ptr()), L.ptr(d_n2.data_ptr()),
                L.ptr(d_s2.data_ptr()), m, 0.01, 4, L.ptr(d_dist.data_ptr()), L.ptr(d_lod.data_ptr()),
                L.ptr(d_sig.data_ptr()), L.ptr(st)))

        def chain():
            m3.ComputeDev(t1, t2, d_cores.data_ptr(), d_axes.data_ptr(), m, d_dist.data_ptr(), d_lod.data_ptr(),
                          d_sig.data_ptr(), d_n1.data_ptr(), d_s1.data_ptr(), d_n2.data_ptr(), d_s2.data_ptr(), stream=st)

        def pierce():
            t1.RayPierceDev(d_cores.data_ptr(), d_unit.data_ptr(), m, RHO, d_pierced.data_ptr(), d_s_min=d_lo.data_ptr(),
                            d_s_max=d_hi.data_ptr(), stream=st)

        lanes = admissible(half, target)
        calls = {"stats1": stats1, "stats2": stats2, "finish": finish, "chain": chain}
        for w in lanes:
            calls["lanes_%d" % w] = env("PCGX_CYL_LANES", str(w), stats1)
        calls["walk"] = env("PCGX_RANGE_WALK", "1", stats1)
        calls["pierce"] = pierce
        ts, ks = {k: [] for k in calls}, {k: [] for k in calls}
        for rep in range(reps + 2):
            for k, fn in calls.items():
                sync()
                t0 = time.perf_counter()
                for _ in range(batch):
                    fn()
                sync()
                ms = (time.perf_counter() - t0) * 1e3 / batch
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                sync()
                if rep >= 2:
                    ts[k].append(ms)
                    ks[k].append(e0.elapsed_time(e1))
        res = {"admissible_lanes": lanes, "slab_bound": 2.0 * half / target + 1.0}
        for k in calls:
            res[k] = {"median_ms": float(np.median(ts[k])), "min_ms": float(np.min(ts[k])), "max_ms": float(np.max(ts[k])),
                      "spread_ms": float(np.max(ts[k]) - np.min(ts[k])), "kernel_median_ms": float(np.median(ks[k])),
                      "kernel_min_ms": float(np.min(ks[k]))}
        # the variants computed the same: counts equal, sums within a summation order's rounding
        stats1()
        sync()
        n_ref, s_ref = d_n1.clone(), d_s1.clone()
        for w in lanes:
            env("PCGX_CYL_LANES", str(w), stats1)()
            sync()
            res["lanes_%d" % w]["same_counts"] = bool(torch.equal(d_n1, n_ref))
            res["lanes_%d" % w]["max_rel_sum_diff"] = float(((d_s1 - s_ref).abs() / s_ref.abs().clamp_min(1e-300)).max())
        stats1()
        chain()
        sync()
        dist = d_dist.cpu().numpy()
        ok = ~np.isnan(dist)
        res["members_mean"] = float(n_ref.double().mean())
        res["cores_with_a_distance"] = int(ok.sum())
        res["significant"] = int(d_sig.sum())
        res["median_distance_moved_half"] = float(np.median(dist[ok & (d_cores[:, 0].cpu().numpy() > 0.5 * WIDTH)]))
        res["median_distance_still_half"] = float(np.median(dist[ok & (d_cores[:, 0].cpu().numpy() < 0.5 * WIDTH)]))
        # ---- what a user can do today, on a sample of cores
        sc = d_cores[:SAMPLE].cpu().numpy()
        d_sa = d_axes[:SAMPLE].double()

        def range_batch():
            offs, nid, _ = t1.RangeBatch(sc, float(np.sqrt(RHO * RHO + half * half) * 1.001))
            owner = torch.from_numpy(np.repeat(np.arange(SAMPLE), np.diff(offs))).to(dev)
            w = d_P1[torch.from_numpy(nid).to(dev)].double() - d_cores[:SAMPLE].double()[owner]
            dv = d_sa[owner]
            a = (w[:, 0] * dv[:, 0] + w[:, 1] * dv[:, 1]) + w[:, 2] * dv[:, 2]
            c = torch.cross(w, dv, dim=1)
            cc = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
            ddv = (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]
            mem = (cc <= (np.float64(np.float32(RHO)) ** 2) * ddv) & (a * a <= (np.float64(np.float32(half)) ** 2) * ddv)
            cnt = torch.zeros(SAMPLE, dtype=torch.int64, device=dev).index_add_(0, owner[mem], torch.ones_like(owner[mem]))
            s1 = torch.zeros(SAMPLE, dtype=torch.float64, device=dev).index_add_(0, owner[mem], a[mem])
            s2 = torch.zeros(SAMPLE, dtype=torch.float64, device=dev).index_add_(0, owner[mem], (a * a)[mem])
            sync()
            return cnt.cpu().numpy(), s1.cpu().numpy(), s2.cpu().numpy(), len(nid)

        rbs = []
        for rep in range(reps + 2):  # the same rounds as the calls: two warm-ups, then a median
            sync()
            t0 = time.perf_counter()
            cnt, _, _, ncand = range_batch()  # (ends in a synchronise and a read-back of the three arrays)
            if rep >= 2:
                rbs.append((time.perf_counter() - t0) * 1e3)
        rb = float(np.median(rbs))
        v = []
        for rep in range(reps + 2):
            sync()
            t0 = time.perf_counter()
            for _ in range(batch):
                t1.CylinderStatsDev(d_cores.data_ptr(), d_axes.data_ptr(), SAMPLE, RHO, half, d_n1.data_ptr(), d_s1.data_ptr(), st)
            sync()
            if rep >= 2:
                v.append((time.perf_counter() - t0) * 1e3 / batch)
        res["range_batch"] = {"sample_cores": SAMPLE, "ms": rb, "min_ms": float(np.min(rbs)), "max_ms": float(np.max(rbs)),
                              "candidates": ncand,
                              "same_counts": bool(np.array_equal(cnt, d_n1[:SAMPLE].cpu().numpy())),
                              "stats_sample_median_ms": float(np.median(v)), "ratio": rb / float(np.median(v))}
        out["by_half_length"]["%g" % half] = res
        print(json.dumps({"half_length": half, **res}), flush=True)
    out["lanes_decision"] = decide(out["by_half_length"])
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
