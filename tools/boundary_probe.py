"""GPU probe: boundary points (csrc/boundary.hip) -- BoundaryDev beside NormalsDev on the same cloud, handle and radius
in the same run: the 1M-point surface cloud at r = 0.1, the normals row of DESIGN.md 3.6.  Both enumerate the same
neighbourhoods; boundary does about twenty float64 operations a neighbour and no eigen-solve.

    python tools/boundary_probe.py [--out profiles/boundary_probe.json] [--reps 11] [--only NAME]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/boundary_probe.py --reps 3 --only NAME
    python tools/boundary_probe.py --trace-summary DIR --only NAME --out profiles/boundary_probe.json   (adds "kernel_trace")

The calls alternate in one process; a timing is a host clock around --batch calls in a row and one device synchronise,
divided by the batch; each repetition times every call in turn after two warm-up rounds; the figures are medians over
--reps rounds, and "spread_ms" (max - min over the rounds) is the run-to-run spread a difference has to exceed.
  normals        NormalsDev, normals alone (no curvature, no counts)
  boundary       BoundaryDev on those normals, every optional output asked for
  boundary_min   ... ids and the count alone
  boundary_walk  ... under PCGX_RANGE_WALK=1 (the tree walk instead of the grid), normals_walk beside it
  maxima         LocalMaximaDev on a random score: the cheapest consumer of the same enumeration
The trace summary sums the kernels of a run by name (run it with --only: one kind of call in the trace): the boundary
kernel and the four compaction launches separately."""
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

RADIUS = 0.1


def measure(reps, batch, only):
    import torch
    from pcgol_amd import build as B
    from pcgol_amd import kdtree, synth
    sync = torch.cuda.synchronize
    P = synth.surface_cloud(1_000_000, 30.0, 6)[0]
    n = len(P)
    t = kdtree.New(P)
    dev, i32 = "cuda", torch.int32
    d_nrm = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    d_ids, d_gaps, d_counts = (torch.zeros(n, dtype=i32, device=dev) for _ in range(3))
    d_masks = torch.zeros(n, dtype=torch.int64, device=dev)
    d_n = torch.zeros(1, dtype=i32, device=dev)
    d_score = torch.from_numpy(np.random.default_rng(1).random(n).astype(np.float32)).to(dev)
    vp = (0.0, 0.0, 100.0)

    def walk(fn):
        def run():
            os.environ["PCGX_RANGE_WALK"] = "1"  # (read per call)
            fn()
            os.environ.pop("PCGX_RANGE_WALK", None)
        return run

    def normals():
        t.NormalsDev(RADIUS, d_nrm.data_ptr(), Viewpoint=vp)

    def boundary():
        t.BoundaryDev(RADIUS, d_nrm.data_ptr(), d_ids.data_ptr(), d_n.data_ptr(), d_gaps.data_ptr(), d_masks.data_ptr(),
                      d_counts.data_ptr())

    def boundary_min():
        t.BoundaryDev(RADIUS, d_nrm.data_ptr(), d_ids.data_ptr(), d_n.data_ptr())

    def maxima():
        t.LocalMaximaDev(RADIUS, d_score.data_ptr(), d_ids.data_ptr(), d_n.data_ptr())

    normals()
    sync()
    calls = {"normals": normals, "boundary": boundary, "boundary_min": boundary_min, "normals_walk": walk(normals),
             "boundary_walk": walk(boundary), "maxima": maxima}
    calls = {k: v for k, v in calls.items() if not only or k == only}
    out = {"points": n, "radius": RADIUS, "reps": reps, "batch": batch}
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
            if rep == 0 and k.startswith("boundary"):
                out[k + "_found"] = int(d_n.cpu()[0])
    if "boundary" in calls:
        boundary()
        sync()
        g = d_gaps.cpu().numpy()
        out["mean_count"] = float(d_counts.cpu().numpy().mean())
        out["gap_histogram"] = np.bincount(g[g >= 0], minlength=65).tolist()
    for k, v in ts.items():
        out[k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                  "spread_ms": float(np.max(v) - np.min(v))}
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
        if not any(s in name for s in ("boundary_", "keypoints_", "normals_", "local_maxima_")):
            continue
        by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/boundary_probe.py --reps 3 --only NAME "
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
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.trace_summary:
        res.setdefault("kernel_trace", {})[a.only or "all"] = trace_summary(a.trace_summary)
    else:
        res.update(measure(a.reps, a.batch, a.only))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
