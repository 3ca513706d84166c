"""GPU probe: FPFH at the keypoints only (pcgx_kdtree_fpfh_at_dev; csrc/fpfh.hip: fpfh_mark_kernel, spfh_kernel<., true>,
fpfh_kernel<., true>) against the path it replaces, FPFHDev over every point plus a torch gather of the keypoints' rows, and
the coarse-alignment chain both ways.

    python tools/fpfh_at_probe.py [--out profiles/fpfh_at_probe.json] [--reps 21]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR_A -- python tools/fpfh_at_probe.py --reps 3 --kernels-only a
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR_B -- python tools/fpfh_at_probe.py --reps 3 --kernels-only b
    python tools/fpfh_at_probe.py --trace-summary DIR_A DIR_B --out profiles/fpfh_at_probe_kernels.json

Cases, both on synth.c4_plane(1_000_000)'s base with descriptor radius 0.1: (a) its ISS
keypoints at radii 0.1 / 0.1; (b) the same with non_max_radius 0.3: fewer keypoints, and a union of neighbourhoods
well below the cloud.  The method is tools/fpfh_probe.py's: host clock around the call and a device synchronise,
everything device resident, the median of --reps timed calls after two warm-up calls; the yardstick and the new call
alternate in one process (A B A B ...), so that drift hits both.  The yardstick knows the keypoint count on the host
beforehand (the read the new call does without is not charged to it).  The capacity of the compact arrays is the
power of two at or below Len() / 16, chosen without looking at the count.  The chain (both clouds: normals, ISS
keypoints, descriptors, correspondences, pose) is timed both ways, the old way with its one read of the two counts."""
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

# (spfh_kernel<k, true> and fpfh_kernel<k, true> are the stages over the needed points and the slots: the trace names
# the template arguments, so the two forms of each kernel stay apart)
KERNELS = ("spfh_kernel", "fpfh_kernel", "fpfh_mark_kernel", "fpfh_need_")
CASES = {"a": ("iss_0.1_0.1", 0.1, 0.1), "b": ("iss_0.1_0.3", 0.1, 0.3)}
R = 0.1


def stats(ts):
    ts = np.asarray(ts)
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()),
            "q1_ms": float(np.percentile(ts, 25)), "q3_ms": float(np.percentile(ts, 75)), "reps": int(len(ts))}


def alternate(fa, fb, reps, sync):
    """A B A B ...: two warm-up rounds, then `reps` timed rounds -> (stats of A, stats of B)"""
    ta, tb = [], []
    for k in range(reps + 2):
        for fn, ts in ((fa, ta), (fb, tb)):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if k >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ta), stats(tb)


def cap_for(n):
    return 1 << (int(n // 16).bit_length() - 1)


class Cloud:
    """a tree, its normals and its keypoints on the device (the library's stream, waited for)"""

    def __init__(self, pts, salient, non_max):
        import torch
        from pcgol_amd import kdtree
        dev = torch.device("cuda", 0)
        self.n = n = len(pts)
        self.t = kdtree.New(pts)
        self.pts = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev)
        self.dn = torch.empty((n, 3), dtype=torch.float32, device=dev)
        self.di = torch.empty(n, dtype=torch.int32, device=dev)
        self.dc = torch.empty(1, dtype=torch.int32, device=dev)
        self.full = torch.empty((n, 33), dtype=torch.float32, device=dev)
        self.cap = cap = cap_for(n)
        self.f = torch.empty((cap, 33), dtype=torch.float32, device=dev)
        self.x = torch.empty((cap, 3), dtype=torch.float32, device=dev)
        self.ns = torch.empty(1, dtype=torch.int32, device=dev)
        self.salient, self.non_max = salient, non_max

    def normals(self, st=0):
        self.t.NormalsDev(R, self.dn.data_ptr(), stream=st)

    def keypoints(self, st=0):
        self.t.ISSKeypointsDev(self.salient, self.non_max, self.di.data_ptr(), self.dc.data_ptr(), stream=st)

    def fpfh_full(self, st=0):
        self.t.FPFHDev(R, self.dn.data_ptr(), self.full.data_ptr(), stream=st)

    def fpfh_at(self, st=0):
        self.t.FPFHAtDev(R, self.dn.data_ptr(), self.di.data_ptr(), self.cap, self.f.data_ptr(), self.x.data_ptr(),
                         d_n_ids=self.dc.data_ptr(), d_n_spfh=self.ns.data_ptr(), stream=st)


def chain(A, B, reps, sync):
    """the coarse-alignment chain on torch's current stream, both ways -> (stats old, stats new, facts)"""
    import torch
    from pcgol_amd import alignment, features
    dev = A.pts.device
    n_hyp, max_dist = 2048, 0.05
    du = torch.from_numpy(alignment.Samples(n_hyp, 3).view(np.int32)).to(dev)
    res_old = torch.empty(alignment.RESULT_WORDS, dtype=torch.int32, device=dev)
    res_new = torch.empty(alignment.RESULT_WORDS, dtype=torch.int32, device=dev)
    cap = A.cap
    src, dst = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    facts = {}

    def old():
        st = torch.cuda.current_stream().cuda_stream
        for c in (A, B):
            c.normals(st)
            c.fpfh_full(st)
            c.keypoints(st)
        na, nb = int(A.dc.cpu()[0]), int(B.dc.cpu()[0])  # the one read
        ka, kb = A.di[:na].long(), B.di[:nb].long()
        fa, fb, pa, pb = A.full[ka].contiguous(), B.full[kb].contiguous(), A.pts[ka].contiguous(), B.pts[kb].contiguous()
        features.CorrespondencesDev(fa.data_ptr(), na, fb.data_ptr(), nb, src.data_ptr(), dst.data_ptr(), cnt.data_ptr(),
                                    MaxRatio=1.0, Mutual=True, stream=st)
        alignment.EstimatePoseDev(pa.data_ptr(), na, pb.data_ptr(), nb, src.data_ptr(), dst.data_ptr(), na, du.data_ptr(),
                                  n_hyp, res_old.data_ptr(), max_dist, d_n_pairs=cnt.data_ptr(), stream=st)
        facts.update(na=na, nb=nb)

    def new():
        st = torch.cuda.current_stream().cuda_stream
        for c in (A, B):
            c.normals(st)
            c.keypoints(st)
            c.fpfh_at(st)
        features.CorrespondencesDev(A.f.data_ptr(), cap, B.f.data_ptr(), cap, src.data_ptr(), dst.data_ptr(), cnt.data_ptr(),
                                    MaxRatio=1.0, Mutual=True, stream=st)
        alignment.EstimatePoseDev(A.x.data_ptr(), cap, B.x.data_ptr(), cap, src.data_ptr(), dst.data_ptr(), cap,
                                  du.data_ptr(), n_hyp, res_new.data_ptr(), max_dist, d_n_pairs=cnt.data_ptr(), stream=st)

    so, sn = alternate(old, new, reps, sync)
    ro, rn = alignment.ReadResult(res_old.cpu().numpy()), alignment.ReadResult(res_new.cpu().numpy())
    facts.update(cap=cap, found_old=ro["found"], found_new=rn["found"], inliers_old=ro["n_inliers"],
                 inliers_new=rn["n_inliers"], same_pose_bits=bool(np.array_equal(ro["pose"].view(np.uint32), rn["pose"].view(np.uint32))))
    return so, sn, facts


def case(key, c4, reps, kernels_only):
    import torch
    name, salient, non_max = CASES[key]
    sync = torch.cuda.synchronize
    A = Cloud(c4["base"], salient, non_max)
    A.normals()
    A.keypoints()
    sync()
    nk = int(A.dc.cpu()[0])
    assert 0 < nk <= A.cap, (nk, A.cap)
    keys = A.di[:nk].long()
    got = {}

    def yardstick():  # the parent's path: every point's row, then the keypoints' rows gathered
        A.fpfh_full(torch.cuda.current_stream().cuda_stream)
        got["rows"] = A.full[keys].contiguous()

    def at():
        A.fpfh_at(torch.cuda.current_stream().cuda_stream)

    stream = torch.cuda.Stream()  # torch's gathers and the library's kernels in one queue
    torch.cuda.set_stream(stream)
    sy, sa = alternate(yardstick, at, reps, sync)
    n_spfh = int(A.ns.cpu()[0])
    out = {"case": name, "points": A.n, "radius": R, "salient_radius": salient, "non_max_radius": non_max, "keypoints": nk,
           "cap": A.cap, "n_spfh": n_spfh, "n_spfh_share": n_spfh / A.n, "fpfh_dev_plus_gather": sy, "fpfh_at_dev": sa,
           "same_bits": bool(torch.equal(got["rows"].view(torch.int32), A.f[:nk].view(torch.int32))),
           "padding_is_zero": bool((A.f[nk:] == 0).all())}
    out["at_faster_by_ms"] = sy["median_ms"] - sa["median_ms"]
    out["faster_beyond_spread"] = bool(sa["max_ms"] < sy["min_ms"])
    if not kernels_only:
        B = Cloud(c4["target"], salient, non_max)
        so, sn, facts = chain(A, B, max(5, reps // 4), sync)
        out["chain_full_fpfh_one_read"] = so
        out["chain_fpfh_at_no_read"] = sn
        out["chain"] = facts
    print(name, json.dumps(out), flush=True)
    return out


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
        threads = int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0)
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        by.setdefault((name.split("(")[0], threads), []).append(us)
    out = []
    for (name, threads), v in sorted(by.items()):
        out.append({"kernel": name, "threads": threads, "dispatches": len(v), "median_us": round(float(np.median(v)), 2),
                    "min_us": round(float(np.min(v)), 2), "max_us": round(float(np.max(v)), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--trace-summary", nargs=2, default=None, metavar=("DIR_A", "DIR_B"))
    ap.add_argument("--kernels-only", default=None, choices=sorted(CASES), help="one case, the two calls only (the traced run)")
    a = ap.parse_args()
    if a.trace_summary:
        res = {"how": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/fpfh_at_probe.py --reps 3 "
                      "--kernels-only a|b (one run per case, no counters in the run); durations from the trace",
               "cases": {CASES[k][0]: trace_summary(d) for k, d in zip("ab", a.trace_summary)}}
    else:
        from pcgol_amd import build as B
        from pcgol_amd import synth
        c4 = synth.c4_plane(1_000_000)
        res = {"source_hash": B.source_hash(), "cases": {}}
        for key in ([a.kernels_only] if a.kernels_only else sorted(CASES)):
            res["cases"][CASES[key][0]] = case(key, c4, a.reps, bool(a.kernels_only))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    else:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
