"""GPU probe: ground segmentation (csrc/ground.hip) -- GroundDev on a 1M-point undulating scene of 200 m x 200 m at cell
0.25 (800 x 800 cells) and 0.5 (400 x 400), over the schedule of tests/ground_scenes.py's hill (half 1, 2, 4, 8, 16 cells),
with PlanesDev for one plane on the same cloud beside it.

    python tools/ground_probe.py [--out profiles/ground_probe.json] [--reps 11] [--only NAME]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ground_probe.py --reps 3 --only NAME
    python tools/ground_probe.py --trace-summary DIR --only NAME --out profiles/ground_probe.json   (adds "kernel_trace")

Workload: 950 000 terrain points z = 0.08 x + 0.5 sin(0.3 y) + 0.4 sin(0.11 x) with 1 cm noise and 50 000 points of
forty boxes 6 x 5 x 3 m standing on it, shuffled.  The calls alternate in one process; a timing is a host clock around
--batch calls in a row and one device synchronise, divided by the batch; each repetition times every call in turn after
two warm-up rounds; the figures are medians over --reps rounds.
  c25, c50            the hill's schedule at cell 0.25 and 0.5, every optional output asked for
  c25_min             ... labels, sizes and ids alone
  c25_loopN           ... with PCGX_GROUND_LOOP_MAX=N: the plain loop up to half-width N (0: doubling for every window,
                      16: the loop for every window) -- what the threshold kGrLoopMax is chosen from
  c25_hN              one window of half-width N by doubling, c25_hN_loop by the plain loop: the cost against h
  gW_hN, gW_hN_loop   the same on a grid of W x W cells (W 2048, 4096: two and four cells of a row a lane), labels,
                      sizes and ids alone
  planes_h256         PlanesDev, one plane from 256 hypotheses, max_dist 0.15, no refit
The trace summary sums the kernels of a run by name (run it with --only: one kind of call in the trace)."""
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

HALF = np.array([1, 2, 4, 8, 16], np.int32)
HEIGHT = np.array([0.15, 0.45, 0.75, 1.35, 2.5], np.float32)
SIDE = 200.0


def scene():
    rng = np.random.default_rng(23)

    def terrain(x, y):
        return 0.08 * x + 0.5 * np.sin(0.3 * y) + 0.4 * np.sin(0.11 * x)
    n = 950_000
    x, y = rng.random(n) * SIDE, rng.random(n) * SIDE
    parts = [np.column_stack([x, y, terrain(x, y) + rng.normal(0, 0.01, n)])]
    for _ in range(40):
        x0, y0 = rng.random(2) * (SIDE - 6)
        bx, by = x0 + rng.random(1250) * 6, y0 + rng.random(1250) * 5
        parts.append(np.column_stack([bx, by, terrain(bx, by) + 0.3 + rng.random(1250) * 2.7]))
    P = np.concatenate(parts).astype(np.float32)
    return np.ascontiguousarray(P[rng.permutation(len(P))])


def measure(reps, batch, only):
    import torch
    from pcgol_amd import build as B
    from pcgol_amd import kdtree
    sync = torch.cuda.synchronize
    P = scene()
    n = len(P)
    t = kdtree.New(P)
    dev, i32 = "cuda", torch.int32
    d_lab, d_ids, d_win = (torch.zeros(n, dtype=i32, device=dev) for _ in range(3))
    d_sz, d_n = torch.zeros(2, dtype=i32, device=dev), torch.zeros(1, dtype=i32, device=dev)
    d_sf = torch.zeros(800 * 800, dtype=torch.float32, device=dev)
    d_hag = torch.zeros(n, dtype=torch.float32, device=dev)
    smp = torch.from_numpy(np.random.default_rng(1).integers(0, 2 ** 32, 3 * 256, dtype=np.uint64).astype(np.uint32)
                           .view(np.int32)).to(dev)
    p_n, p_sz, p_rf, p_bs = (torch.zeros(1, dtype=i32, device=dev) for _ in range(4))
    p_pl = torch.zeros((1, 4), dtype=torch.float32, device=dev)

    def ground(cell, half=HALF, height=HEIGHT, full=True, loop=None):
        dims = (int(SIDE / cell), int(SIDE / cell))

        def run():
            if loop is None:
                os.environ.pop("PCGX_GROUND_LOOP_MAX", None)
            else:
                os.environ["PCGX_GROUND_LOOP_MAX"] = str(loop)  # (read per call)
            t.GroundDev(cell, half, height, (0.0, 0.0), dims, d_lab.data_ptr(), d_sz.data_ptr(), d_ids.data_ptr(),
                        d_n.data_ptr(), d_window=d_win.data_ptr() if full else 0, d_surface=d_sf.data_ptr() if full else 0,
                        d_hag=d_hag.data_ptr() if full else 0)
        return run

    def planes():
        t.PlanesDev(0.15, smp.data_ptr(), 256, p_n.data_ptr(), p_pl.data_ptr(), p_sz.data_ptr(), p_rf.data_ptr(),
                    p_bs.data_ptr(), d_lab.data_ptr(), d_ids=d_ids.data_ptr(), MaxPlanes=1, MinInliers=3, Refine=False)

    calls = {"c25": ground(0.25), "c50": ground(0.5), "c25_min": ground(0.25, full=False)}
    for lm in (0, 2, 4, 8, 16):
        calls["c25_loop%d" % lm] = ground(0.25, loop=lm)
    for h in (4, 16, 64, 128, 256, 1024, 4096):
        calls["c25_h%d" % h] = ground(0.25, [h], [1.0], loop=0)
    for h in (4, 16, 64, 128, 256):
        calls["c25_h%d_loop" % h] = ground(0.25, [h], [1.0], loop=8192)
    for g in (2048, 4096):  # rows of two and four cells a lane
        for h in (4, 8, 16, 32, 64, 128):
            calls["g%d_h%d" % (g, h)] = ground(SIDE / g, [h], [1.0], full=False, loop=0)
            calls["g%d_h%d_loop" % (g, h)] = ground(SIDE / g, [h], [1.0], full=False, loop=8192)
    calls["planes_h256"] = planes
    calls = {k: v for k, v in calls.items() if not only or k == only}
    out = {"points": n, "half": HALF.tolist(), "height": [float(v) for v in HEIGHT], "reps": reps, "batch": batch}
    ts = {k: [] for k in calls}
    for rep in range(reps + 2):
        for k, fn in calls.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(batch):
                fn()
            sync()
            if rep >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3 / batch)
            if rep == 0:
                out[k + "_found"] = {"sizes": (p_sz if k.startswith("planes") else d_sz).cpu().tolist()}
    os.environ.pop("PCGX_GROUND_LOOP_MAX", None)
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
        if "ground_" not in name and "planes_" not in name:
            continue
        by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/ground_probe.py --reps 3 --only NAME "
                  "(no counters in the run); durations from the trace by kernel name, warm-up launches included",
           "kernels": {}}
    for name, v in sorted(by.items()):
        out["kernels"][name] = {"launches": len(v), "total_us": round(float(np.sum(v)), 1),
                                "median_us": round(float(np.median(v)), 2), "max_us": round(float(np.max(v)), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--batch", type=int, default=20)
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
        res = measure(a.reps, a.batch, a.only)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
