"""GPU probe: cluster extraction (csrc/cluster.hip) -- ClustersDev, Euclidean and with normals and curvature -- with
RegionGrowing.Components over a constant property on the same handle beside it as the yardstick, from the same process.

    python tools/cluster_probe.py [--out profiles/cluster_probe.json] [--reps 11]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cluster_probe.py --reps 3
    python tools/cluster_probe.py --trace-summary DIR --out profiles/cluster_probe.json   (adds "kernel_trace" to the file)

Workloads: the 1M-point base of synth.c2_knn() at r = 0.15 (13.9 neighbours per point), and the base of
synth.c4_plane(1_000_000) at r = 0.075; normals and curvature are the library's (NormalsDev at the same radius, not
timed), MinCos 0.9, MaxCurvature the median curvature.  Four calls alternate in one process:
  (a) region_growing   RegionGrowing.Components with a constant property: host arrays, its upload, download and widening
                       included (the call has no device form)
  (b) clusters_dev     ClustersDev, Euclidean, every output
  (c) clusters_dev_normals   ClustersDev with normals and curvature, every output (half the points are above the
                       median curvature and enumerate nothing)
  (d) clusters_dev_normals_every_edge   ClustersDev with the same normals, oriented, MinCos -2 and no curvature: (b)'s
                       graph (but for the few points without a normal), every candidate's 16-byte record read and
                       tested -- what the extra bytes cost by themselves
Each repetition times every call in turn (host clock around the call and a device synchronise, the method of
tools/ndt_probe.py), after two warm-up rounds; the figures are medians over --reps rounds.

The trace summary cuts the dispatch stream into calls (a call starts at uf_init_kernel or cl_init_kernel; (b) shows in
the edge policy of its rgraph_grid_kernel, ClusterEdge<0>; (c) and (d) run the same kernels, ClusterEdge<2>, and go by
their order in a round) and sums each call's kernels by stage, so the pointer-jumping kernel both source files launch
under one name is counted for the call it ran in.
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

KERNELS = ("cl_", "rg_", "rgraph_", "uf_", "rs_")
CALLS = ("region_growing", "clusters_dev", "clusters_dev_normals", "clusters_dev_normals_every_edge")


def workloads():
    from pcgol_amd import synth
    return [("c2_base_1M_r0.15", synth.c2_knn()["base"], 0.15), ("c4_plane_1M_r0.075", synth.c4_plane(1_000_000)["base"], 0.075)]


def measure(reps):
    import torch
    from pcgol_amd import build as B
    from pcgol_amd import kdtree, segmentation
    sync = torch.cuda.synchronize
    cases = {}
    for name, base, r in workloads():
        base = np.ascontiguousarray(base[:, :3] if base.ndim == 2 else base, np.float32)
        n = len(base)
        t = kdtree.New(base)
        dn = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        dc = torch.empty(n, dtype=torch.float32, device="cuda")
        cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        t.NormalsDev(r, dn.data_ptr(), dc.data_ptr(), cnt.data_ptr())
        sync()
        max_c = float(torch.nanmedian(dc).item())
        lab, siz, ids = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
        c = torch.zeros(1, dtype=torch.int32, device="cuda")
        rg = segmentation.RegionGrowing(t, np.zeros(n, np.uint32))
        res = {}

        def region_growing():
            rg._comp.clear()  # (Components caches per range)
            res["rg"] = rg.Components(r)

        def clusters_dev():
            t.ClustersDev(r, lab.data_ptr(), c.data_ptr(), siz.data_ptr(), ids.data_ptr())

        def clusters_dev_normals():
            t.ClustersDev(r, lab.data_ptr(), c.data_ptr(), siz.data_ptr(), ids.data_ptr(), d_normals=dn.data_ptr(), MinCos=0.9,
                          d_curvature=dc.data_ptr(), MaxCurvature=max_c)

        def clusters_dev_normals_every_edge():
            t.ClustersDev(r, lab.data_ptr(), c.data_ptr(), siz.data_ptr(), ids.data_ptr(), d_normals=dn.data_ptr(), MinCos=-2.0,
                          Oriented=True)

        calls = dict(zip(CALLS, (region_growing, clusters_dev, clusters_dev_normals, clusters_dev_normals_every_edge)))
        ts = {k: [] for k in calls}
        out = {"points": n, "radius": r, "neighbours_per_point": float(cnt.float().mean().item()), "max_curvature": max_c,
               "reps": reps}
        for rep in range(reps + 2):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                sync()
                if rep >= 2:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
                if rep == 0 and k != "region_growing":
                    out[k + "_clusters"] = int(c.item())
                    out[k + "_largest"] = siz[:3].cpu().tolist()
                    out[k + "_unlabelled"] = int((lab < 0).sum().item())
                    if k == "clusters_dev":  # the same partition as the yardstick's
                        names = torch.from_numpy(res["rg"]).cuda()
                        first = ids[torch.cumsum(siz[:int(c.item())].long(), 0) - siz[:int(c.item())].long()].long()
                        out["same_partition_as_region_growing"] = bool(torch.equal(first[lab.long()], names))
        for k, v in ts.items():
            out[k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
        out["normals_over_euclidean"] = out["clusters_dev_normals"]["median_ms"] / out["clusters_dev"]["median_ms"]
        out["normals_every_edge_over_euclidean"] = (out["clusters_dev_normals_every_edge"]["median_ms"] /
                                                    out["clusters_dev"]["median_ms"])
        print(json.dumps({name: out}), flush=True)
        cases[name] = out
        del t, rg
    return {"source_hash": B.source_hash(), "cases": cases}


def stage_of(name, seen_rank, seen_label):
    if "rgraph_grid_kernel" in name or "rgraph_walk_kernel" in name or "uf_jump_kernel" in name:
        return "components"
    if "cl_init_kernel" in name or "cl_stage_" in name:
        return "staging"
    if "cl_root_stats_kernel" in name or "cl_name_kernel" in name:
        return "sizes_and_names"
    if "rg_min_id_kernel" in name or "rg_name_kernel" in name or "uf_init_kernel" in name:
        return "naming"
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
    rows = [r for r in rows if any(s in r.get("Kernel_Name", "") for s in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = []  # {"kind", stage: us}
    cur = None
    for r in rows:
        name = r["Kernel_Name"].split("(")[0]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "uf_init_kernel" in name or "cl_init_kernel" in name:
            cur = {"kind": CALLS[0] if "uf_init_kernel" in name else None, "stages": {}, "rank": False, "label": False}
            calls.append(cur)
        if cur is None:
            continue  # (sorts of the tree builds before the first call)
        if "rgraph_grid_kernel" in name and "ClusterEdge" in name:
            if "ClusterEdge<2>" not in name:
                cur["kind"] = CALLS[1]
            elif cur["kind"] is None:  # (c) and (d) run the same kernels: (c) follows (b), (d) follows (c)
                prev = [c["kind"] for c in calls[:-1] if c["kind"]]
                cur["kind"] = CALLS[3] if prev and prev[-1] == CALLS[2] else CALLS[2]
        st = stage_of(name, cur["rank"], cur["label"])
        cur["label"] = cur["label"] or "cl_label_kernel" in name
        if cur["kind"] == CALLS[0] and st not in ("components", "naming"):
            continue  # (a tree build's sort behind a region growing call)
        cur["stages"][st] = cur["stages"].get(st, 0.0) + us
        if "cl_ids_kernel" in name or "rg_name_kernel" in name:
            cur = None  # the call's last kernel (what follows may be the next workload's tree build)
    calls = [c for c in calls if c["kind"]]
    half = len(calls) // 2
    out = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/cluster_probe.py --reps 3 (no "
                  "counters in the run); durations from the trace, summed per call and stage; the first two rounds of a "
                  "workload are warm-up and left out", "cases": {}}
    for (wname, _, _), part in zip(workloads_names(), (calls[:half], calls[half:])):
        case = {}
        for kind in CALLS:
            mine = [c["stages"] for c in part if c["kind"] == kind][2:]
            stages = sorted({s for c in mine for s in c})
            case[kind] = {"calls": len(mine)}
            for s in stages:
                v = [c.get(s, 0.0) for c in mine]
                case[kind][s + "_us"] = {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2),
                                         "max": round(float(np.max(v)), 2)}
        a, b = case[CALLS[0]].get("components_us"), case[CALLS[1]].get("components_us")
        if a and b:
            case["components_b_minus_a_us"] = round(b["median"] - a["median"], 2)
            case["components_a_spread_us"] = round(a["max"] - a["min"], 2)
        out["cases"][wname] = case
    return out


def workloads_names():
    return [("c2_base_1M_r0.15", None, None), ("c4_plane_1M_r0.075", None, None)]


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
