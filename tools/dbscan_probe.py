"""GPU probe: density clustering (csrc/dbscan.hip over csrc/cluster.hip) -- DBSCANDev at min_pts 1, 8, 15 and 30, the flag
pass with and without its early stop -- with ClustersDev (Euclidean) on the same handle beside it as the yardstick, from
the same process.

    python tools/dbscan_probe.py [--out profiles/dbscan_probe.json] [--reps 11]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/dbscan_probe.py --reps 3
    python tools/dbscan_probe.py --trace-summary DIR --out profiles/dbscan_probe.json   (adds "kernel_trace" to the file)

Workloads: the two 1M-point clouds of tools/cluster_probe.py (the base of synth.c2_knn() at r = 0.15, the base of
synth.c4_plane(1_000_000) at r = 0.075).  Eight calls alternate in one process, every output asked for:
  clusters_dev            ClustersDev, Euclidean: the yardstick
  dbscan_1                DBSCANDev at min_pts 1: the same launches and one scatter of kind
  dbscan_M, dbscan_M_count_all   for M in 8, 15, 30: DBSCANDev with the flag pass stopping at min_pts, and
                          (PCGX_DBSCAN_COUNT_ALL=1) counting the whole neighbourhood
Each repetition times every call in turn (host clock around the call and a device synchronise, the method of
tools/cluster_probe.py), after two warm-up rounds; the figures are medians over --reps rounds.  The yardstick's own
spread between repetitions stands beside dbscan_1's difference from it.

The trace summary cuts the dispatch stream into calls (a call starts at cl_init_kernel; the calls of a round come in
the order above) and sums each call's kernels by stage."""
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

MIN_PTS = (8, 15, 30)
CALLS = ("clusters_dev", "dbscan_1") + tuple("dbscan_%d%s" % (m, s) for m in MIN_PTS for s in ("", "_count_all"))
NAMES = ("c2_base_1M_r0.15", "c4_plane_1M_r0.075")


def workloads():
    from pcgol_amd import synth
    return [(NAMES[0], synth.c2_knn()["base"], 0.15), (NAMES[1], synth.c4_plane(1_000_000)["base"], 0.075)]


def measure(reps):
    import torch
    from pcgol_amd import build as B
    from pcgol_amd import kdtree
    sync = torch.cuda.synchronize
    cases = {}
    for name, base, r in workloads():
        base = np.ascontiguousarray(base[:, :3] if base.ndim == 2 else base, np.float32)
        n = len(base)
        t = kdtree.New(base)
        lab, siz, ids = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
        kind = torch.empty(n, dtype=torch.uint8, device="cuda")
        c = torch.zeros(1, dtype=torch.int32, device="cuda")

        def clusters_dev():
            t.ClustersDev(r, lab.data_ptr(), c.data_ptr(), siz.data_ptr(), ids.data_ptr())

        def dbscan(m, count_all=False):
            def run():
                if count_all:
                    os.environ["PCGX_DBSCAN_COUNT_ALL"] = "1"
                try:
                    t.DBSCANDev(r, m, lab.data_ptr(), c.data_ptr(), siz.data_ptr(), ids.data_ptr(), kind.data_ptr())
                finally:
                    os.environ.pop("PCGX_DBSCAN_COUNT_ALL", None)
            return run

        fns = [clusters_dev, dbscan(1)] + [dbscan(m, a) for m in MIN_PTS for a in (False, True)]
        calls = dict(zip(CALLS, fns))
        ts = {k: [] for k in calls}
        out = {"points": n, "radius": r, "reps": reps}
        first = {}
        for rep in range(reps + 2):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                sync()
                if rep >= 2:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
                if rep == 0:
                    first[k] = (lab.clone(), int(c.item()), siz.clone(), ids.clone(), kind.clone())
                    out[k + "_clusters"] = int(c.item())
                    out[k + "_largest"] = siz[:3].cpu().tolist()
                    if k != "clusters_dev":
                        out[k + "_core_border_noise"] = [int((kind == v).sum().item()) for v in (2, 1, 0)]
        a, b = first["clusters_dev"], first["dbscan_1"]
        out["dbscan_1_equals_clusters_dev"] = bool(a[1] == b[1] and all(torch.equal(a[i], b[i]) for i in (0, 2, 3)))
        for m in MIN_PTS:  # the early stop changes no bit
            a, b = first["dbscan_%d" % m], first["dbscan_%d_count_all" % m]
            out["dbscan_%d_same_bits_both_ways" % m] = bool(a[1] == b[1] and all(torch.equal(a[i], b[i]) for i in (0, 2, 3, 4)))
        for k, v in ts.items():
            out[k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
        y = out["clusters_dev"]
        out["dbscan_1_minus_clusters_dev_ms"] = out["dbscan_1"]["median_ms"] - y["median_ms"]
        out["clusters_dev_spread_ms"] = y["max_ms"] - y["min_ms"]
        for m in MIN_PTS:
            out["dbscan_%d_over_clusters_dev" % m] = out["dbscan_%d" % m]["median_ms"] / y["median_ms"]
            out["dbscan_%d_stop_over_count_all" % m] = (out["dbscan_%d" % m]["median_ms"] /
                                                        out["dbscan_%d_count_all" % m]["median_ms"])
        print(json.dumps({name: out}), flush=True)
        cases[name] = out
        del t
    return {"source_hash": B.source_hash(), "cases": cases}


def stage_of(name, seen_label):
    if "db_flag_" in name:
        return "flag_pass"
    if "db_border_" in name:
        return "border_pass"
    if "db_kind_kernel" in name:
        return "kind"
    if "rgraph_grid_kernel" in name or "rgraph_walk_kernel" in name or "uf_jump_kernel" in name:
        return "components"
    if "cl_init_kernel" in name or "cl_stage_" in name:
        return "staging"
    if "cl_root_stats_kernel" in name or "cl_name_kernel" in name:
        return "sizes_and_names"
    if "rs_" in name:
        return "sort_2" if seen_label else "sort_1"
    if "cl_rank_kernel" in name or "cl_label_kernel" in name:
        return "ranking"
    if "cl_ids_kernel" in name:
        return "grouping"
    return "other"


def trace_summary(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows = [r for r in rows if any(s in r.get("Kernel_Name", "") for s in ("cl_", "db_", "rgraph_", "uf_", "rs_"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        name = r["Kernel_Name"].split("(")[0]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "cl_init_kernel" in name:
            cur = {"stages": {}, "label": False}
            calls.append(cur)
        if cur is None:
            continue  # (sorts of the tree builds before the first call)
        st = stage_of(name, cur["label"])
        cur["label"] = cur["label"] or "cl_label_kernel" in name
        cur["stages"][st] = cur["stages"].get(st, 0.0) + us
        if "cl_ids_kernel" in name:
            cur = None  # the call's last kernel (what follows may be the next workload's tree build)
    half = len(calls) // 2
    out = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/dbscan_probe.py --reps 3 (no "
                  "counters in the run); durations from the trace, summed per call and stage; the first two rounds of a "
                  "workload are warm-up and left out", "cases": {}}
    for wname, part in zip(NAMES, (calls[:half], calls[half:])):
        case = {}
        for i, kind in enumerate(CALLS):
            mine = [c["stages"] for c in part[i::len(CALLS)]][2:]
            case[kind] = {"calls": len(mine)}
            for s in sorted({s for c in mine for s in c}):
                v = [c.get(s, 0.0) for c in mine]
                case[kind][s + "_us"] = {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2),
                                         "max": round(float(np.max(v)), 2)}
        out["cases"][wname] = case
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
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
