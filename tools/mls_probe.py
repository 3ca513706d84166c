"""GPU probe: moving-least-squares smoothing (pcgx_kdtree_mls_dev, csrc/mls.hip) at order 1 and order 2 against
pcgx_kdtree_normals_dev on the same handle -- the yardstick: order 1 is the normals kernel's enumeration and solve with
another finish, order 2 enumerates twice and adds an exp and 28 float64 FMAs per neighbour.

    python tools/mls_probe.py [--out profiles/mls_probe.json] [--reps 21]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mls_probe.py --reps 3
    python tools/mls_probe.py --trace-summary DIR --out profiles/mls_probe.json     (adds "kernels" to the file)

Workload: the base of synth.c4_plane(1_000_000) (1M surface points, width 30), q == NULL (the tree's own points),
radius = sigma = 0.1, ~34 neighbours each, everything device resident.  The three calls alternate in one process: each
repetition times normals, order 1, order 2 in turn (host clock around the call and a device synchronise), after two
warm-up rounds; the figures are medians over --reps rounds.  The kernels' own durations come from one separate
kernel-trace run with no counters.
"""
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

KERNELS = ("mls_kernel", "normals_kernel")


def measure(reps):
    import torch
    from pcgol_amd import build as B
    from pcgol_amd import kdtree, synth
    base = synth.c4_plane(1_000_000)["base"]
    r = 0.1
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    t = kdtree.New(base)
    n = len(base)
    dp = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dn = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dc = torch.empty(n, dtype=torch.float32, device=dev)
    dkind = torch.empty(n, dtype=torch.int32, device=dev)
    dk = torch.empty(n, dtype=torch.int32, device=dev)
    sync()
    calls = {
        "normals_dev": lambda: t.NormalsDev(r, dn.data_ptr(), dc.data_ptr(), dk.data_ptr()),
        "mls_dev_order1": lambda: t.MLSDev(r, dp.data_ptr(), dn.data_ptr(), dkind.data_ptr(), dk.data_ptr(), Order=1),
        "mls_dev_order2": lambda: t.MLSDev(r, dp.data_ptr(), dn.data_ptr(), dkind.data_ptr(), dk.data_ptr(), Order=2),
    }
    ts = {k: [] for k in calls}
    for rep in range(reps + 2):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            sync()
            if rep >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    out = {"points": n, "own_points": True, "radius": r, "sigma": r, "reps": reps}
    for k, v in ts.items():
        out[k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
    kinds = dkind.cpu().numpy()  # (of the last call: order 2)
    out["mean_neighbours"] = float(dk.cpu().numpy().mean())
    out["kinds_order2"] = np.bincount(kinds, minlength=3).tolist()
    out["order1_over_normals"] = out["mls_dev_order1"]["median_ms"] / out["normals_dev"]["median_ms"]
    out["order2_over_normals"] = out["mls_dev_order2"]["median_ms"] / out["normals_dev"]["median_ms"]
    print(json.dumps(out), flush=True)
    return {"source_hash": B.source_hash(), "cases": {"surface_1M_own_r0.1": out}}


def trace_summary(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    by = {}
    for r in rows:
        name = r.get("Kernel_Name", "")
        if not any(s in name for s in KERNELS):
            continue
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        by.setdefault(name.split("(")[0], []).append(us)
    out = []
    for name, v in sorted(by.items()):
        out.append({"kernel": name, "dispatches": len(v), "median_us": round(float(np.median(v)), 2),
                    "min_us": round(float(np.min(v)), 2), "max_us": round(float(np.max(v)), 2)})
    med = {k["kernel"]: k["median_us"] for k in out}
    ratios = {}
    base = next((v for k, v in med.items() if "normals_kernel" in k), None)
    for k, v in med.items():
        if base and "mls_kernel" in k:
            ratios[k + " / normals_kernel"] = round(v / base, 3)
    return {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/mls_probe.py --reps 3 (no counters "
                   "in the run); durations from the trace", "kernels": out, "ratios": ratios}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--trace-summary", default=None)
    a = ap.parse_args()
    if a.trace_summary:
        res = {}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        res["kernel_trace"] = trace_summary(a.trace_summary)
    else:
        res = measure(a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
