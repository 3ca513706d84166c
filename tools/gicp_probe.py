"""GPU probe: the Generalized ICP step (csrc/icp.hip, icp_gicp_sums_kernel behind the correspondence kernels) against
the point-to-plane step of the same run on the same scene -- the yardstick: the same correspondence phase, with the
30 sums formed inside it from one float4 normal per pair instead of by a pass of their own over the covariances.

    python tools/gicp_probe.py [--out profiles/gicp_probe.json] [--reps 11] [--trace-only]
    python tools/gicp_probe.py --trace-summary DIR --out profiles/gicp_probe.json   (merges kernel times into --out)

Case: synth.c4_plane(1_000_000) (1M surface points, target = T * base[perm]), everything device resident.
  step_ms          one timed window is FITS (50) Fits of 20 iterations each, enqueued back to back behind resets, and
                   one device synchronise (about 0.1 s), host clock, / (FITS * 20); the GICP and the plane session
                   alternate inside every repetition (A / B in one process); median of --reps windows after two
                   warm-up windows of each.  window_ms is recorded beside it.
  covariances_ms   pcgx_kdtree_covariances_dev (k = 20, PLANE) of the base and of the target, each call + synchronise.
  fit_knn_ms       the whole pcgx_icp_gicp_fit_knn call from host arrays: target tree build, both covariance calls, the
                   session, 20 iterations, the result.
--trace-only runs three GICP Fits and three plane Fits and nothing else: the target of
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/gicp_probe.py --trace-only`; --trace-summary DIR then reads
that run's kernel_trace.csv files and adds the kernels' own durations (icp_gicp_sums_kernel among them) to --out.
bytes_per_target is the algorithm's: point 12, target covariance 24, pair 16 + 4, partner's covariance 32 gathered."""
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

BYTES_PER_TARGET = 12 + 24 + 16 + 4 + 32
COPY_CEILING_TBS = 6.29  # float4 device copy, measured (MI355X)
ITERS = 20
FITS = 50  # Fits per timed window


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "reps": len(ts)}


def scene():
    import torch
    from pcgol_amd import icp, kdtree, synth
    c = synth.c4_plane(1_000_000)
    dev = torch.device("cuda", 0)
    t = kdtree.New(c["base"])
    tt = kdtree.New(c["target"])
    n = len(c["base"])
    d = {"target": torch.from_numpy(c["target"]).to(dev), "normals": torch.from_numpy(c["normals"]).to(dev),
         "bc": torch.empty((n, 6), dtype=torch.float32, device=dev), "tc": torch.empty((n, 6), dtype=torch.float32, device=dev)}
    torch.cuda.synchronize()
    th = np.full(6, -1, np.float32)
    mk = dict(gicp=lambda: icp.IcpSession(t, d["target"].data_ptr(), c["max_dist"], 6, None, th, ITERS, target_on_device=True,
                                          nt=n, BaseCov=d["bc"], TargetCov=d["tc"]),
              plane=lambda: icp.IcpSession(t, d["target"].data_ptr(), c["max_dist"], 6, None, th, ITERS, target_on_device=True,
                                           nt=n, BaseNormals=d["normals"]))
    return c, t, tt, d, mk


def fit(s):
    s.reset()
    for _ in range(ITERS):
        s.step()


def probe(reps):
    import torch
    from pcgol_amd import icp
    sync = torch.cuda.synchronize
    c, t, tt, d, mk = scene()
    out = {"points": len(c["base"]), "iterations": ITERS, "bytes_per_target": BYTES_PER_TARGET}
    cov = {"base": [], "target": []}
    for rep in range(reps + 2):
        for name, tree, buf in (("base", t, d["bc"]), ("target", tt, d["tc"])):
            sync()
            t0 = time.perf_counter()
            tree.CovariancesDev(20, buf.data_ptr())
            sync()
            if rep >= 2:
                cov[name].append((time.perf_counter() - t0) * 1e3)
    out["covariances_ms"] = {k: stats(v) for k, v in cov.items()}
    sess = {k: f() for k, f in mk.items()}
    ts = {k: [] for k in sess}
    for rep in range(reps + 2):
        for k, s in sess.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(FITS):
                fit(s)
            sync()
            if rep >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3 / (ITERS * FITS))
    out["step_ms"] = {k: stats(v) for k, v in ts.items()}
    out["window_ms"] = {k: float(np.median(v)) * ITERS * FITS for k, v in ts.items()}
    out["fits_per_window"] = FITS
    out["gicp_over_plane"] = out["step_ms"]["gicp"]["median_ms"] / out["step_ms"]["plane"]["median_ms"]
    res = {k: s.result() for k, s in sess.items()}
    out["num_iteration"] = {k: int(r[1].NumIteration) for k, r in res.items()}
    out["dropped"] = int(sess["gicp"].dropped())
    for s in sess.values():
        s.close()
    reg = icp.GeneralizedICP.FromKNN(c["max_dist"], K=20, Epsilon=1e-3, MinPairs=6,
                                     UpdaterFactory=icp.GaussNewtonUpdaterFactory(Threshold=np.full(6, -1, np.float32),
                                                                                  MaxIteration=ITERS))
    tk = []
    for rep in range(max(3, reps // 3) + 1):
        t0 = time.perf_counter()
        reg.Fit(t, c["target"])
        if rep >= 1:
            tk.append((time.perf_counter() - t0) * 1e3)
    out["fit_knn_ms"] = stats(tk)
    return out


def trace_only():
    import torch
    c, t, tt, d, mk = scene()
    for tree, buf in ((t, d["bc"]), (tt, d["tc"])):
        tree.CovariancesDev(20, buf.data_ptr())
    for k, f in mk.items():
        s = f()
        for _ in range(3):
            fit(s)
        s.result()
        s.close()
    torch.cuda.synchronize()


def trace_summary(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    by = {}
    for r in rows:
        name = r.get("Kernel_Name", "")
        if not any(s in name for s in ("icp_", "knearest_kernel")):
            continue
        by.setdefault(name.split("(")[0], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = []
    for name, v in sorted(by.items()):
        v = np.sort(np.array(v))
        out.append({"kernel": name, "dispatches": len(v), "median_us": round(float(np.median(v)), 2),
                    "min_us": round(float(v[0]), 2), "max_us": round(float(v[-1]), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--trace-summary", default=None)
    a = ap.parse_args()
    if a.trace_only:
        trace_only()
        return
    from pcgol_amd import build as B
    if a.trace_summary:
        res = {}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        ks = trace_summary(a.trace_summary)
        res["kernels"] = {"how": "rocprofv3 --kernel-trace --stats -- python tools/gicp_probe.py --trace-only (no counters in "
                                 "the run); durations from the trace; an iteration past `done` returns at once: medians",
                          "rows": ks}
        g = [k for k in ks if "icp_gicp_sums_kernel" in k["kernel"]]
        if g:
            us = g[0]["median_us"]
            n = res.get("points", 1_000_000)
            tbs = BYTES_PER_TARGET * n / (us * 1e-6) / 1e12
            res["gicp_sums_kernel"] = {"median_us": us, "algorithmic_TB_per_s": round(tbs, 3),
                                       "share_of_copy_ceiling": round(tbs / COPY_CEILING_TBS, 3),
                                       "copy_ceiling_TB_per_s": COPY_CEILING_TBS}
    else:
        res = {"source_hash": B.source_hash()}
        res.update(probe(a.reps))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
