"""Plane and shape segmentation share their round machinery (csrc/consensus_peel.h): PlanesDev, ShapesDev, PlanesDev,
ShapesDev enqueued on one tree and one stream with nothing read back in between give what each call gives alone -- no
state of the rounds is shared between the two models, or between two calls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_scenes as PS  # noqa: E402
import shape_scenes as SC  # noqa: E402

pytestmark = pytest.mark.gpu
u32 = np.uint32
N_HYP, ROUNDS = 128, 2


def test_planes_and_shapes_interleaved_on_one_stream():
    import torch
    from pcgol_amd import kdtree
    P, M, part = SC.yard()
    t = kdtree.KDTree(P)
    n = len(P)
    dev = torch.device("cuda", 0)
    i32 = torch.int32
    d_nrm = torch.from_numpy(M).to(dev)
    cyl, sph = SC.CALLS["cylinders"], SC.CALLS["spheres"]

    def shape_kw(c):
        kw = c[1]
        return dict(MinInliers=600, MinNormalCos=0.8, SampleRadius=kw["sample_radius"], RMin=kw["r_min"], RMax=kw["r_max"])

    # (what, samples, record width, keyword arguments): the floor; the poles; the floor again, by its normals; the ball
    calls = [("planes", PS.samples(N_HYP, ROUNDS, 11), 4, dict(MinInliers=600, Refine=False)),
             ("shapes", SC.samples(N_HYP, ROUNDS, SC.SEEDS[0]), 8, dict(Kind=cyl[0], Refine=True, **shape_kw(cyl))),
             ("planes", PS.samples(N_HYP, ROUNDS, 12), 4, dict(MinInliers=600, Refine=True, MinNormalCos=0.8,
                                                               d_normals=d_nrm.data_ptr())),
             ("shapes", SC.samples(N_HYP, ROUNDS, SC.SEEDS[1]), 8, dict(Kind=sph[0], Refine=False, **shape_kw(sph)))]
    d_smp = [torch.from_numpy(np.ascontiguousarray(s, u32).reshape(-1).view(np.int32).copy()).to(dev) for _, s, _, _ in calls]

    def outputs(rec):
        # n_found, sizes, refined, best, labels, ids, status, counts; records, hyp -- filled with rubbish
        ints = [torch.full((k,), -7, dtype=i32, device=dev) for k in (1, ROUNDS, ROUNDS, ROUNDS, n, n, ROUNDS * N_HYP,
                                                                      ROUNDS * N_HYP)]
        return ints, [torch.full((k, rec), 7.0, dtype=torch.float32, device=dev) for k in (ROUNDS, ROUNDS * N_HYP)]

    def enqueue(k, out, stream):
        what, _, _, kw = calls[k]
        (d_n, d_sz, d_rf, d_bs, d_lab, d_ids, d_st, d_cn), (d_rec, d_hyp) = out
        opt = dict(d_ids=d_ids.data_ptr(), d_status=d_st.data_ptr(), d_counts=d_cn.data_ptr(), stream=stream)
        if what == "planes":
            t.PlanesDev(0.02, d_smp[k].data_ptr(), N_HYP, d_n.data_ptr(), d_rec.data_ptr(), d_sz.data_ptr(), d_rf.data_ptr(),
                        d_bs.data_ptr(), d_lab.data_ptr(), d_hyp_planes=d_hyp.data_ptr(), MaxPlanes=ROUNDS, **opt, **kw)
        else:
            kw = dict(kw)
            t.ShapesDev(kw.pop("Kind"), 0.02, d_nrm.data_ptr(), d_smp[k].data_ptr(), N_HYP, d_n.data_ptr(), d_rec.data_ptr(),
                        d_sz.data_ptr(), d_rf.data_ptr(), d_bs.data_ptr(), d_lab.data_ptr(), d_hyp_shapes=d_hyp.data_ptr(),
                        MaxShapes=ROUNDS, **opt, **kw)

    def read(out):
        return [x.cpu().numpy().view(u32) for x in out[0] + out[1]]

    s = torch.cuda.Stream()
    alone = []
    for k in range(len(calls)):
        out = outputs(calls[k][2])
        torch.cuda.synchronize()
        enqueue(k, out, s.cuda_stream)
        torch.cuda.synchronize()
        alone.append(read(out))
    assert all(int(a[0][0]) >= 1 for a in alone)  # every call finds something: the floor, poles, the floor, the ball
    together = [outputs(c[2]) for c in calls]
    torch.cuda.synchronize()
    for k in range(len(calls)):
        enqueue(k, together[k], s.cuda_stream)  # nothing is read back, nothing is waited for
    torch.cuda.synchronize()
    for k, out in enumerate(together):
        for i, (a, b) in enumerate(zip(alone[k], read(out))):
            assert np.array_equal(a, b), (k, calls[k][0], i)
