"""GPU probe: farthest-point sampling (pcgx_kdtree_fps_dev; csrc/fps.hip) against its yardsticks, alternated in one run.

    python tools/fps_probe.py [--out profiles/fps_probe.json] [--reps 11]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fps_probe.py --one-call 1000000 4096
    python tools/fps_probe.py --trace-last-call DIR --out profiles/fps_probe_kernels.json

Shapes: synth.surface_cloud(1_000_000, 30, 6) at count 64, 1024, 4096 and 16 384, and a 16 384-point cloud at count
1024 (the point-network shape).  Per shape, one call of each after the other, --reps times after two warm-up rounds:
  fps_dev        FarthestPointsDev with every output (a wide launch per pick: the only form in the tree);
  prep           the call's preparation alone (pcgx_kdtree_fps_prep_dev): gather, Morton order, tiles;
  torch_loop     what a user does without the library: d = torch.minimum(d, ((P - P[i]) ** 2).sum(1)); i = d.argmax()
                 on the same device, no host synchronise inside the loop;
  thin_dev       ThinDev at the radius sqrt(cover_sq) of the 4096-pick result (1M shapes), of this shape's (16 384).
Each figure is the median and range of the timed calls, host clock around the call, ending in a device synchronise.
The touched tiles per pick come from the counter pcgx_kdtree_fps_prep_dev fills in a run of its own; the per-kernel
split from the traced run of one call.  (profiles/fps_probe_narrow.json is this probe's output on the build that had a
one-workgroup kernel for the late picks, alternated with wide-only: the comparison that took that kernel out.)"""
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


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "reps": len(ts)}


def alternated(fns, reps, sync):
    """{name: fn}: every fn once per round, two warm-up rounds, then reps timed rounds"""
    ts = {k: [] for k in fns}
    for rep in range(reps + 2):
        for k, fn in fns.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if rep >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: summary(v) for k, v in ts.items()}


class Cloud:
    def __init__(self, pts):
        import torch
        from pcgol_amd import kdtree
        self.dev = torch.device("cuda", 0)
        self.pts = pts
        self.n = len(pts)
        self.t = kdtree.New(pts)
        self.P = torch.from_numpy(pts).to(self.dev)
        self.own = torch.empty(self.n, dtype=torch.int32, device=self.dev)
        self.thin_ids = torch.empty(self.n, dtype=torch.int32, device=self.dev)
        self.words = torch.zeros(4, dtype=torch.int32, device=self.dev)

    def fps(self, count, bufs):
        ids, m, dsq, cov = bufs
        self.t.FarthestPointsDev(count, ids.data_ptr(), m.data_ptr(), dsq.data_ptr(), cov.data_ptr(), self.own.data_ptr())

    def touched(self, count):
        """tiles touched per pick, from the device counter"""
        import torch
        from pcgol_amd import _lib as L
        c = torch.zeros(count, dtype=torch.int32, device=self.dev)
        L.check(L.lib().pcgx_kdtree_fps_prep_dev(self.t._h, count, L.ptr(int(c.data_ptr())), None))
        torch.cuda.synchronize()
        return c.cpu().numpy().astype(np.int64)

    def bufs(self, count):
        import torch
        return (torch.empty(count, dtype=torch.int32, device=self.dev), torch.zeros(1, dtype=torch.int32, device=self.dev),
                torch.empty(count, dtype=torch.float32, device=self.dev), torch.zeros(1, dtype=torch.float32, device=self.dev))

    def torch_loop(self, count, out):
        import torch
        P = self.P
        d = torch.full((self.n,), float("inf"), device=self.dev)
        i = torch.zeros((), dtype=torch.int64, device=self.dev)
        for j in range(count):
            out[j] = i
            d = torch.minimum(d, ((P - P[i]) ** 2).sum(1))
            i = d.argmax()

    def thin(self, r):
        w = self.words.data_ptr()
        self.t.ThinDev(r, self.thin_ids.data_ptr(), w, w + 4, Seed=1)


def shape(c, count, reps, thin_radius=None):
    import torch
    from pcgol_amd import _lib as L
    sync = torch.cuda.synchronize
    bufs = c.bufs(count)
    loop_ids = torch.empty(count, dtype=torch.int64, device=c.dev)
    c.fps(count, bufs)
    sync()
    cover = float(bufs[3].cpu()[0])
    r = thin_radius if thin_radius is not None else float(np.sqrt(cover))
    fns = {"fps_dev": lambda: c.fps(count, bufs),
           "prep": lambda: L.check(L.lib().pcgx_kdtree_fps_prep_dev(c.t._h, count, None, None)),
           "torch_loop": lambda: c.torch_loop(count, loop_ids),
           "thin_dev": lambda: c.thin(r)}
    out = {"points": c.n, "count": count, "cover_sq": cover, "thin_radius": r}
    out.update(alternated(fns, reps, sync))
    picks = out["fps_dev"]["median_ms"] - out["prep"]["median_ms"]
    out["per_pick_us"] = 1e3 * picks / count
    plan = np.zeros(4, np.int64)
    L.check(L.lib().pcgx_fps_plan(c.n, count, L.ptr(plan)))
    out["plan"] = {"tiles": int(plan[1]), "wg_tiles": int(plan[2]), "workgroups": int(plan[3])}
    tt = c.touched(count)
    out["touched_tiles"] = {"first8": tt[:8].tolist(), "mean_steps_8_to_63": float(tt[8:64].mean()) if count > 8 else None,
                            "mean_from_step_64": float(tt[64:].mean()) if count > 64 else None,
                            "mean_last_256": float(tt[-256:].mean()), "max": int(tt.max()), "mean": float(tt.mean())}
    out["torch_loop_per_pick_us"] = 1e3 * out["torch_loop"]["median_ms"] / count
    out["ratio_torch_loop_to_fps"] = out["torch_loop"]["median_ms"] / out["fps_dev"]["median_ms"]
    out["thin_kept"] = int(c.words.cpu()[0])
    # the torch loop squares in float32 in another order and breaks ties its own way: how far its picks agree
    a, b = bufs[0].cpu().numpy().astype(np.int64), loop_ids.cpu().numpy()
    out["torch_loop_same_picks"] = int((a == b).sum())
    print(json.dumps(out), flush=True)
    return out, cover


def one_call(n, count):
    """warm-up calls, then ONE FarthestPointsDev with every output and nothing behind it: the traced run whose last
    call --trace-last-call lists"""
    import torch
    from pcgol_amd import synth
    pts = np.ascontiguousarray(synth.surface_cloud(n, 30.0 if n > 100_000 else 4.0, 6)[0], np.float32)
    c = Cloud(pts)
    bufs = c.bufs(count)
    for _ in range(3):
        torch.cuda.synchronize()
        c.fps(count, bufs)
    torch.cuda.synchronize()
    print(json.dumps({"points": c.n, "count": count, "n_ids": int(bufs[1].cpu()[0])}))


def trace_last_call(d):
    """the dispatches from the last fps_gather_kernel on, in start order: one call"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    last = max(k for k, r in enumerate(rows) if "fps_gather_kernel" in r["Kernel_Name"])
    rows = rows[last:]
    end = max(k for k, r in enumerate(rows) if "fps_finish_kernel" in r["Kernel_Name"])
    rows = rows[:end + 1]
    name = lambda r: r["Kernel_Name"].split("(")[0].replace("void ", "").replace("pcgx::", "")  # noqa: E731
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    picks = [r for r in rows if name(r).startswith("fps_pick_kernel")]
    pv = np.array([us(r) for r in picks])
    starts = np.array([int(r["Start_Timestamp"]) for r in picks])
    ends = np.array([int(r["End_Timestamp"]) for r in picks])
    gaps = (starts[1:] - ends[:-1]) / 1e3
    other = {}
    for r in rows:
        if not name(r).startswith("fps_pick_kernel"):
            other[name(r)] = round(other.get(name(r), 0.0) + us(r), 2)
    first = int(rows[0]["Start_Timestamp"])
    out = {"dispatches": len(rows), "span_us": round((int(rows[-1]["End_Timestamp"]) - first) / 1e3, 1),
           "pick_launches": len(picks), "other_kernels_us": other}
    if len(picks):
        out.update({"prep_span_us": round((starts[0] - first) / 1e3, 1),
                    "pick_kernel_mean_us": round(float(pv.mean()), 2), "pick_kernel_median_us": round(float(np.median(pv)), 2),
                    "pick_kernel_first8_us": [round(float(v), 2) for v in pv[:8]],
                    "pick_kernel_last_quarter_mean_us": round(float(pv[-max(len(pv) // 4, 1):].mean()), 2)})
    if len(picks) > 1:
        out.update({"gap_between_picks_mean_us": round(float(gaps.mean()), 2),
                    "gap_between_picks_median_us": round(float(np.median(gaps)), 2),
                    "pick_start_to_start_mean_us": round(float(np.diff(starts).mean() / 1e3), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--one-call", type=int, nargs=2, default=None, metavar=("POINTS", "COUNT"))
    ap.add_argument("--trace-last-call", default=None, nargs="+", help="trace directories, one per traced --one-call run")
    a = ap.parse_args()
    if a.one_call is not None:
        return one_call(*a.one_call)
    if a.trace_last_call:
        res = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/fps_probe.py --one-call POINTS "
                      "COUNT (no counters in the run): the last call of the run, every output, its pick launches",
               "calls": {os.path.basename(os.path.normpath(d)): trace_last_call(d) for d in a.trace_last_call}}
    else:
        from pcgol_amd import build as B
        from pcgol_amd import synth
        res = {"source_hash": B.source_hash(), "shapes": {}}
        big = Cloud(np.ascontiguousarray(synth.surface_cloud(1_000_000, 30.0, 6)[0], np.float32))
        _, cover = shape(big, 4096, 1)  # (the radius the 1M shapes hand to ThinDev)
        r = float(np.sqrt(cover))
        for count in (64, 1024, 4096, 16384):
            res["shapes"]["surface_1M_count_%d" % count] = shape(big, count, a.reps, r)[0]
        del big
        small = Cloud(np.ascontiguousarray(synth.surface_cloud(16384, 4.0, 6)[0], np.float32))
        res["shapes"]["surface_16384_count_1024"] = shape(small, 1024, a.reps)[0]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
