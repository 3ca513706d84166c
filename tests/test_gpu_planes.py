"""Plane segmentation on the GPU (KDTree.Planes / PlanesDev, csrc/planes.hip) against the NumPy restatement of its contract
(tests/plane_oracle.py).  Rule of every case: the integer outputs are array_equal to the oracle evaluated at the library's
own hyp_planes; hyp_planes are equal to the oracle's by uint32 view; a refitted plane is the contract's formula applied to
KDTree.GroupStats of the library's own pre-refinement inliers (the oracle is given that GroupStats); the padding is
checked; a second call gives the first call's bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_oracle as PO  # noqa: E402
import plane_scenes as SC  # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
INT_FIELDS = ("n_planes", "sizes", "refined", "best", "labels", "ids", "status", "counts")


@pytest.fixture(scope="module")
def K():
    from pcgol_amd import kdtree
    return kdtree


@pytest.fixture(scope="module")
def room(K):
    P = SC.room()
    return P, K.KDTree(P)


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def same(a, b):
    for f in a._fields:
        x, y = getattr(a, f), getattr(b, f)
        assert np.array_equal(bits(x), bits(y)) if np.asarray(x).dtype == f32 else np.array_equal(x, y), f


def check(K, t, P, smp, max_dist, n_hyp, deleted=None, **kw):
    """Planes on the host form against the oracle -> (library result, oracle result)."""
    names = dict(max_planes="MaxPlanes", min_inliers="MinInliers", axis="Axis", min_axis_cos="MinAxisCos", normals="Normals",
                 min_normal_cos="MinNormalCos", refine="Refine")
    args = {names[k]: v for k, v in kw.items()}
    got = t.Planes(max_dist, NHyp=n_hyp, Samples=smp, **args)
    want = PO.segment(P, smp, max_dist, n_hyp, deleted=deleted, hyp_planes=got.hyp_planes, group_stats=PO.library_frame(t),
                      **kw)
    for f in INT_FIELDS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), (f, getattr(got, f), getattr(want, f))
    assert np.array_equal(bits(got.hyp_planes), bits(want.hyp_planes))
    assert np.array_equal(bits(got.planes), bits(want.planes))
    assert got.labels.dtype == np.int64 and len(got.labels) == len(P)
    same(got, t.Planes(max_dist, NHyp=n_hyp, Samples=smp, **args))
    return got, want


def planes_dev(K, t, smp, max_dist, n_hyp, max_planes=1, normals=None, want=("ids", "status", "counts", "hyp_planes"),
               **kw):
    """The device form over torch tensors filled with rubbish -> the same tuple, ids with their padding."""
    import torch
    dev = torch.device("cuda", 0)
    n, rows = t.Len(), max(n_hyp * max_planes, 1)
    i32 = torch.int32
    d_smp = torch.from_numpy(np.ascontiguousarray(smp, u32).reshape(-1).view(np.int32).copy()).to(dev)
    d_n, d_sz, d_rf, d_bs = (torch.full((k,), -7, dtype=i32, device=dev) for k in (1, max_planes, max_planes, max_planes))
    d_pl = torch.full((max_planes, 4), 7.0, dtype=torch.float32, device=dev)
    d_lab, d_ids = (torch.full((max(n, 1),), -7, dtype=i32, device=dev) for _ in range(2))
    d_st, d_cn = (torch.full((rows,), -7, dtype=i32, device=dev) for _ in range(2))
    d_hp = torch.full((rows, 4), 7.0, dtype=torch.float32, device=dev)
    d_nrm = torch.from_numpy(np.ascontiguousarray(normals, f32)).to(dev) if normals is not None else None
    opt = dict(ids=d_ids, status=d_st, counts=d_cn, hyp_planes=d_hp)
    ptr = {k: (v.data_ptr() if k in want else 0) for k, v in opt.items()}
    torch.cuda.synchronize()
    t.PlanesDev(max_dist, d_smp.data_ptr() if n_hyp else 0, n_hyp, d_n.data_ptr(), d_pl.data_ptr(), d_sz.data_ptr(),
                d_rf.data_ptr(), d_bs.data_ptr(), d_lab.data_ptr(), d_ids=ptr["ids"], d_status=ptr["status"],
                d_counts=ptr["counts"], d_hyp_planes=ptr["hyp_planes"], MaxPlanes=max_planes,
                d_normals=d_nrm.data_ptr() if d_nrm is not None else 0,
                stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    c = lambda x: x.cpu().numpy()  # noqa: E731
    return K.PlaneSegments(int(c(d_n)[0]), c(d_pl), c(d_sz).astype(np.int64), c(d_rf), c(d_bs).astype(np.int64),
                           c(d_lab)[:n].astype(np.int64), c(d_ids)[:n].astype(np.int64), c(d_st)[:n_hyp * max_planes],
                           c(d_cn)[:n_hyp * max_planes].astype(np.int64), c(d_hp)[:n_hyp * max_planes])


def same_as_host(dev, host, n):
    k = len(host.ids)
    assert np.array_equal(dev.ids[:k], host.ids) and np.all(dev.ids[k:] == -1) and len(dev.ids) == n  # the padding
    assert dev.n_planes == host.n_planes
    for f in ("sizes", "refined", "best", "labels"):
        assert np.array_equal(getattr(dev, f), getattr(host, f)), f
    assert np.array_equal(dev.status, host.status.reshape(-1)) and np.array_equal(dev.counts, host.counts.reshape(-1))
    assert np.array_equal(bits(dev.planes), bits(host.planes))
    assert np.array_equal(bits(dev.hyp_planes), bits(host.hyp_planes.reshape(-1, 4)))


@pytest.fixture
def split(monkeypatch):
    def set_split(v):
        if v is None:
            monkeypatch.delenv("PCGX_PLANES_SPLIT", raising=False)
        else:
            monkeypatch.setenv("PCGX_PLANES_SPLIT", str(v))
    return set_split


@pytest.mark.parametrize("n_hyp", [128, 256])
def test_room_peels_four_planes_and_stops(K, room, n_hyp):
    P, t = room
    smp = SC.samples(n_hyp, 6, 11)
    first = PO.segment(P, smp, 0.02, n_hyp, max_planes=6, min_inliers=600)  # the scene does what it is for
    assert first.n_planes == 4 and 0 < first.counts[4].max() < 200
    got, want = check(K, t, P, smp, 0.02, n_hyp, max_planes=6, min_inliers=600)
    assert got.n_planes == 4 and np.all(got.status[4] >= 0) and np.all(got.status[5] == -1)
    assert np.all(got.counts[5] == 0) and np.all(got.hyp_planes[5] == 0)
    assert got.sizes[4:].tolist() == [0, 0] and got.best[4:].tolist() == [-1, -1] and np.all(got.planes[4:] == 0)
    assert all(abs(int(s) - w) < 0.06 * w for s, w in zip(got.sizes, (6000, 3000, 2000, 1200)))
    # a refined plane (whether a round's refit loses no inlier is the scene's business: test_refinement_rules has both) is the contract's formula on GroupStats of the library's own pre-refinement inliers
    for r in np.flatnonzero(got.refined):
        g = t.GroupStats(want.pre_ids[r], [len(want.pre_ids[r])])
        ok, pl = PO.refit(g.centroid[0], g.axes[0, 2], g.eig[0, 0])
        assert ok and np.array_equal(bits(pl), bits(got.planes[r]))


def test_room_every_split_both_forms_and_deleted(K, room, split):
    P, t = room
    n_hyp = 128
    smp = SC.samples(n_hyp, 6, 12)
    split(None)
    host = t.Planes(0.02, NHyp=n_hyp, MaxPlanes=6, MinInliers=600, Samples=smp)
    assert host.n_planes == 4
    for s in (1, 3, len(P) + 5):
        split(s)
        same(host, t.Planes(0.02, NHyp=n_hyp, MaxPlanes=6, MinInliers=600, Samples=smp))
    same_as_host(planes_dev(K, t, smp, 0.02, n_hyp, max_planes=6, MinInliers=600), host, len(P))
    split(None)
    same_as_host(planes_dev(K, t, smp, 0.02, n_hyp, max_planes=6, MinInliers=600), host, len(P))
    # each optional output NULL: the others do not change
    for leave in ("ids", "status", "counts", "hyp_planes"):
        d = planes_dev(K, t, smp, 0.02, n_hyp, max_planes=6, MinInliers=600,
                       want=tuple(k for k in ("ids", "status", "counts", "hyp_planes") if k != leave))
        assert np.all(np.asarray(getattr(d, leave)).reshape(-1) == (7 if leave == "hyp_planes" else -7))  # untouched
        assert d.n_planes == 4 and np.array_equal(d.labels, host.labels) and np.array_equal(bits(d.planes), bits(host.planes))
        if leave != "ids":
            assert np.array_equal(d.ids[:len(host.ids)], host.ids)
    # a handle with a tenth of its ids deleted: never sampled, never inliers
    td = K.KDTree(P)
    gone = np.random.default_rng(2).permutation(len(P))[:len(P) // 10]
    td.DeletePoints(gone)
    deleted = np.zeros(len(P), bool)
    deleted[gone] = True
    for s in (None, 3):
        split(s)
        got, _ = check(K, td, P, smp, 0.02, n_hyp, deleted=deleted, max_planes=6, min_inliers=540)
        assert got.n_planes == 4 and np.all(got.labels[gone] == -1) and not np.isin(got.ids, gone).any()
    same_as_host(planes_dev(K, td, smp, 0.02, n_hyp, max_planes=6, MinInliers=540), got, len(P))


def test_launch_boundaries(K, room):
    P, t = room
    tile = K.PlanesTile()
    assert tile == 128
    part = P[:3000]
    tp = K.KDTree(part)
    for n_hyp in (1, tile - 1, tile, tile + 1, 2 * tile + 1):
        got, _ = check(K, tp, part, SC.samples(n_hyp, 2, n_hyp), 0.02, n_hyp, max_planes=2, min_inliers=50)
        assert n_hyp < 64 or got.n_planes == 2
    rng = np.random.default_rng(4)
    for n in (1, 2, 3, 63, 64, 65, 257, 1024, 1025):
        Q = (rng.random((n, 3)) * (1, 1, 0.01)).astype(f32)
        got, _ = check(K, K.KDTree(Q), Q, SC.samples(40, 3, n), 0.02, 40, max_planes=3)
        if n < 3:
            assert got.n_planes == 0 and np.all(got.status == -1) and np.all(got.labels == -1)
        else:
            assert got.n_planes >= 1 and got.sizes[0] >= 3 and got.status[0].max() >= 0
        if n == 3:
            assert got.sizes.tolist() == [3, 0, 0] and np.all(got.status[1:] == -1)  # R_1 = 0: the round cannot run


def test_strict_less_and_the_tie(K):
    P = SC.lattice(0.125)
    t = K.KDTree(P)
    tri = [(0, 9, 60), (3, 40, 21), (64, 73, 124), (3, 40, 21), (0, 64, 9)]
    got, _ = check(K, t, P, SC.words(tri, 128), 0.125, 5, refine=False)
    assert got.counts[0].tolist() == [64, 64, 64, 64, 44] and got.best.tolist() == [0]
    assert np.array_equal(got.ids, np.arange(64)) and got.planes[0].tolist() == [0, 0, 1, 0]
    got, _ = check(K, t, P, SC.words(tri[4:] + tri[1:4], 128), float(np.nextafter(f32(0.125), f32(1))), 4, refine=False)
    assert got.counts[0].tolist() == [44, 128, 128, 128] and got.best.tolist() == [1]  # the duplicated triple: the smaller h
    got, _ = check(K, t, P, np.tile(SC.words(tri[:1], 128), (2, 1)), 0.125, 1, max_planes=2, refine=True)
    assert got.n_planes == 2 and got.sizes.tolist() == [64, 64] and np.array_equal(got.ids, np.arange(128))


def test_axis(K, room):
    P, t = room
    n_hyp = 256
    smp = SC.samples(n_hyp, 1, 13)
    c10 = float(np.cos(np.radians(10)))
    free, _ = check(K, t, P, smp, 0.02, n_hyp, min_inliers=600)
    got, _ = check(K, t, P, smp, 0.02, n_hyp, min_inliers=600, axis=(0, 0, 1), min_axis_cos=c10)
    assert (got.status[0] == 3).sum() > (free.status[0] == 0).sum() // 2 and not (free.status == 3).any()
    assert got.n_planes == 1 and got.planes[0, 2] > 0.999 and abs(got.sizes[0] - 6000) < 360  # the floor
    assert np.all(got.hyp_planes[0][got.status[0] == 0][:, 2] >= c10 - 1e-6)
    got, _ = check(K, t, P, smp, 0.02, n_hyp, min_inliers=600, axis=(-1, 0, 0), min_axis_cos=c10)
    assert got.n_planes == 1 and got.planes[0, 0] < -0.999 and abs(got.sizes[0] - 3000) < 180  # the wall x = 0, turned to -x
    assert np.all(got.hyp_planes[0][got.status[0] == 0][:, 0] < 0)


def test_normals_keep_the_feet_of_the_box_out(K):
    P, M = SC.box_on_floor()
    t = K.KDTree(P)
    smp = SC.samples(128, 1, 14)
    plain, po = check(K, t, P, smp, 0.02, 128, min_inliers=1000)
    withn, wo = check(K, t, P, smp, 0.02, 128, min_inliers=1000, normals=M, min_normal_cos=0.9)
    assert po.sizes[0] - wo.sizes[0] > 0 and plain.sizes[0] - withn.sizes[0] == po.sizes[0] - wo.sizes[0]
    feet = np.setdiff1d(plain.ids, withn.ids)
    assert len(feet) > 10 and np.all(np.abs(M[feet, 2]) < 0.5) and np.all(np.abs(M[withn.ids, 2]) >= 0.9)
    same_as_host(planes_dev(K, t, smp, 0.02, 128, normals=M, MinInliers=1000, MinNormalCos=0.9), withn, len(P))
    # zero and NaN normals: such a point takes no part
    M2 = M.copy()
    M2[::7] = 0
    M2[3::7, 1] = np.nan
    got, _ = check(K, t, P, smp, 0.02, 128, min_inliers=500, normals=M2, min_normal_cos=0.9)
    assert got.n_planes == 1 and np.all(got.labels[::7] == -1) and np.all(got.labels[3::7] == -1)


def test_refinement_rules(K):
    P, w = SC.refit_loses()
    t = K.KDTree(P)
    off, _ = check(K, t, P, w, 0.02, 1, refine=False)
    on, want = check(K, t, P, w, 0.02, 1, refine=True)
    g = t.GroupStats(np.arange(14), [14])
    ok, pl = PO.refit(g.centroid[0], g.axes[0, 2], g.eig[0, 0])
    assert ok and PO.inlier_mask(pl, P, 0.02).sum() == 13  # the refit loses the low point: the hypothesis is kept
    assert on.refined.tolist() == [0] and on.sizes.tolist() == [14] and np.array_equal(bits(on.planes), bits(off.planes))
    Q = P.copy()
    Q[13, 2] = 0.019
    tq = K.KDTree(Q)
    on, want = check(K, tq, Q, w, 0.02, 1, refine=True)
    off, _ = check(K, tq, Q, w, 0.02, 1, refine=False)
    assert on.refined.tolist() == [1] and off.refined.tolist() == [0] and on.sizes.tolist() == [14]
    assert off.planes[0].tolist() == [0, 0, 1, 0] and -0.019 < on.planes[0, 3] < -0.005
    g = tq.GroupStats(want.pre_ids[0], [14])
    assert np.array_equal(bits(PO.refit(g.centroid[0], g.axes[0, 2], g.eig[0, 0])[1]), bits(on.planes[0]))
    # three inliers, nearly on a line (sin^2 of their angle at 4e-12): group geometry fits them a frame all the same (its
    # trace is not 0), and whether that refit is kept is the count's business: the oracle, given GroupStats, says which
    T = np.array([[0, 0, 0], [1, 0, 0], [2, 4e-6, 0], [0, 0, 9], [1, 1, 9], [3, 0, 9.5]], f32)
    got, _ = check(K, K.KDTree(T), T, SC.words([(0, 1, 2)], 6), 1e-4, 1, refine=True)
    assert got.status.tolist() == [[0]] and got.sizes.tolist() == [3]


def test_edges_of_the_contract(K):
    rng = np.random.default_rng(7)
    n_hyp = 40
    smp = SC.samples(n_hyp, 2, 15)
    nanc = np.full((100, 3), np.nan, f32)
    got, _ = check(K, K.KDTree(nanc), nanc, smp, 0.02, n_hyp, max_planes=2)
    assert got.n_planes == 0 and np.all(got.status == -1) and np.all(got.labels == -1) and len(got.ids) == 0
    Q = (rng.random((600, 3)) * (1, 1, 0.005)).astype(f32)
    Q[::5, 0] = np.inf
    Q[1::5, 2] = np.nan
    Q[2::50] = -np.inf
    t = K.KDTree(Q)
    got, _ = check(K, t, Q, smp, 0.02, n_hyp, max_planes=2)
    assert got.n_planes == 1 and np.all(got.labels[::5] == -1) and np.all(got.labels[1::5] == -1)
    assert got.sizes[0] == np.isfinite(Q).all(axis=1).sum()
    t.DeletePoints(np.arange(len(Q)))  # every point deleted
    got, _ = check(K, t, Q, smp, 0.02, n_hyp, max_planes=2, deleted=np.ones(len(Q), bool))
    assert got.n_planes == 0 and np.all(got.status == -1)
    # every hypothesis rejected: the round ran, found nothing, and the next one does not run
    L = np.column_stack([np.arange(50), np.arange(50), np.arange(50)]).astype(f32)
    got, _ = check(K, K.KDTree(L), L, smp, 0.02, n_hyp, max_planes=2)
    assert got.n_planes == 0 and set(got.status[0].tolist()) <= {1, 2} and np.all(got.status[1] == -1)
    assert got.best.tolist() == [-1, -1] and np.all(got.counts == 0)
    # n_hyp == 0 is fine and finds nothing, on both forms
    t = K.KDTree(Q)
    got = t.Planes(0.02, NHyp=0, MaxPlanes=3)
    assert got.n_planes == 0 and np.all(got.labels == -1) and got.best.tolist() == [-1] * 3 and got.status.shape == (3, 0)
    d = planes_dev(K, t, smp, 0.02, 0, max_planes=3)
    assert d.n_planes == 0 and np.all(d.labels == -1) and np.all(d.ids == -1) and d.best.tolist() == [-1] * 3
    assert np.all(d.sizes == 0) and np.all(d.planes == 0) and np.all(d.refined == 0)
    # (a tree of no points cannot be built -- pcgx_kdtree_build refuses it -- so Len() == 0 has no test)


def test_invalid_arguments_write_nothing(K, room):
    import ctypes as C
    from pcgol_amd import _lib as L
    P, t = room
    smp = SC.samples(8, 2, 1)
    nan = float("nan")
    bad = [dict(NHyp=-1), dict(MaxPlanes=0), dict(MaxPlanes=257), dict(MaxDist=0.0), dict(MaxDist=-1.0),
           dict(MaxDist=float("inf")), dict(MaxDist=nan), dict(MinInliers=-1), dict(Axis=(0, 0, 0)), dict(Axis=(0, nan, 1)),
           dict(Axis=(np.inf, 0, 1)), dict(Axis=(0, 0, 1), MinAxisCos=1.5), dict(Axis=(0, 0, 1), MinAxisCos=-0.1),
           dict(Axis=(0, 0, 1), MinAxisCos=nan), dict(Normals=np.ones_like(P), MinNormalCos=1.01),
           dict(Normals=np.ones_like(P), MinNormalCos=nan)]
    for kw in bad:
        a = dict(MaxDist=0.02, NHyp=8, MaxPlanes=2, Samples=smp)
        a.update(kw)
        with pytest.raises((L.PcgxError, ValueError)):
            t.Planes(a.pop("MaxDist"), **a)
    # an unused bound is not checked: no axis, no normals
    assert t.Planes(0.02, NHyp=8, MaxPlanes=2, Samples=smp, MinAxisCos=7.0, MinNormalCos=-3.0).n_planes >= 0
    # ... and nothing is written: the raw call with rubbish in every output
    n = len(P)
    out = [np.full(k, 77, d) for k, d in ((8, f32), (2, np.int64), (2, np.int32), (2, np.int64), (n, np.int64), (n, np.int64),
                                          (16, np.int32), (16, np.int64), (64, f32))]
    cnt = C.c_int64(77)
    lib = L.lib()

    def raw(tree=t._h, samples=L.ptr(smp), n_hyp=8, mp=2, md=0.02, skip=None):
        ptrs = [None if i == skip else L.ptr(a) for i, a in enumerate(out)]
        return lib.pcgx_kdtree_planes(tree, samples, n_hyp, mp, md, 3, None, 0.0, None, 0.0, 1, C.byref(cnt), *ptrs)
    calls = [dict(tree=None), dict(samples=None), dict(mp=300), dict(md=nan), dict(n_hyp=-2),
             dict(n_hyp=2 ** 24, mp=256)] + [dict(skip=i) for i in range(5)]
    for kw in calls:
        assert raw(**kw) == L.PCGX_E_INVALID, kw
        assert cnt.value == 77 and all(np.all(a == 77) for a in out), kw
    assert lib.pcgx_kdtree_planes(t._h, L.ptr(smp), 8, 2, 0.02, 3, None, 0.0, None, 0.0, 1, None, *[L.ptr(a) for a in out]) \
        == L.PCGX_E_INVALID
    assert raw(skip=5) == L.PCGX_OK and np.all(out[5] == 77) and cnt.value != 77  # ids may be NULL


def test_the_chain_on_one_stream(K, room):
    """PlanesDev -> a torch mask -> ClustersDev -> GroupStatsDev -> GroupHullsDev on one stream, no synchronise in
    between; then PlaneSegmentation's Extract, Boxes and Footprints: equal to the host forms."""
    import torch
    from pcgol_amd import segmentation
    P, t = room
    n, n_hyp, mp = len(P), 128, 6
    dev = torch.device("cuda", 0)
    i32, f64 = torch.int32, torch.float64
    smp = SC.samples(n_hyp, mp, 0)
    host = t.Planes(0.02, NHyp=n_hyp, MaxPlanes=mp, MinInliers=600, Samples=smp)
    d_smp = torch.from_numpy(smp.reshape(-1).view(np.int32).copy()).to(dev)
    d_n, d_sz, d_rf, d_bs = (torch.full((k,), -7, dtype=i32, device=dev) for k in (1, mp, mp, mp))
    d_pl = torch.zeros((mp, 4), dtype=torch.float32, device=dev)
    d_lab, d_ids, c_lab, c_sz, c_ids = (torch.full((n,), -7, dtype=i32, device=dev) for _ in range(5))
    c_n = torch.full((1,), -7, dtype=i32, device=dev)
    g_cnt = torch.zeros(mp, dtype=i32, device=dev)
    g_cen, g_axes, g_obb = (torch.zeros((mp, k), dtype=f64, device=dev) for k in (3, 9, 6))
    h_sz = torch.zeros(mp, dtype=i32, device=dev)
    h_ids = torch.full((n,), -7, dtype=i32, device=dev)
    h_area, h_rect = torch.zeros(mp, dtype=f64, device=dev), torch.zeros((mp, 6), dtype=f64, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t.PlanesDev(0.02, d_smp.data_ptr(), n_hyp, d_n.data_ptr(), d_pl.data_ptr(), d_sz.data_ptr(), d_rf.data_ptr(),
                    d_bs.data_ptr(), d_lab.data_ptr(), d_ids=d_ids.data_ptr(), MaxPlanes=mp, MinInliers=600,
                    stream=s.cuda_stream)
        on_plane = (d_lab >= 0).float()
        t.ClustersDev(0.12, c_lab.data_ptr(), c_n.data_ptr(), c_sz.data_ptr(), c_ids.data_ptr(),
                      d_curvature=on_plane.data_ptr(), MaxCurvature=0.5, MinSize=1, stream=s.cuda_stream)
        t.GroupStatsDev(d_ids.data_ptr(), n, d_sz.data_ptr(), mp, d_n_groups=d_n.data_ptr(), d_count=g_cnt.data_ptr(),
                        d_centroid=g_cen.data_ptr(), d_axes=g_axes.data_ptr(), d_obb=g_obb.data_ptr(), stream=s.cuda_stream)
        t.GroupHullsDev(d_ids.data_ptr(), n, d_sz.data_ptr(), mp, d_n_groups=d_n.data_ptr(), d_hull_sizes=h_sz.data_ptr(),
                        d_hull_ids=h_ids.data_ptr(), d_area=h_area.data_ptr(), d_rect=h_rect.data_ptr(),
                        stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert int(d_n[0]) == host.n_planes == 4 and np.array_equal(d_lab.cpu().numpy(), host.labels)
    assert np.array_equal(d_sz.cpu().numpy(), host.sizes) and np.array_equal(d_ids.cpu().numpy()[:len(host.ids)], host.ids)
    # the clusters of what is on no plane, as the host form finds them with the same mask
    lab, sizes, ids = t.Clusters(0.12, Curvature=(host.labels >= 0).astype(f32), MaxCurvature=0.5)
    assert int(c_n[0]) == len(sizes) and np.array_equal(c_lab.cpu().numpy(), lab)
    assert np.all(lab[host.labels >= 0] == -1) and np.all(lab[host.labels < 0] >= 0)
    geo, feet = t.GroupStats(host.ids, host.sizes[:4]), t.GroupHulls(host.ids, host.sizes[:4])
    assert np.array_equal(g_cnt.cpu().numpy()[:4], geo.count) and np.array_equal(g_cen.cpu().numpy()[:4], geo.centroid)
    assert np.array_equal(g_axes.cpu().numpy()[:4].reshape(4, 3, 3), geo.axes) and np.array_equal(g_obb.cpu().numpy()[:4], geo.obb)
    assert np.array_equal(h_sz.cpu().numpy()[:4], feet.hull_sizes) and np.array_equal(h_area.cpu().numpy()[:4], feet.area)
    assert np.array_equal(h_rect.cpu().numpy()[:4], feet.rect) and np.all(g_cnt.cpu().numpy()[4:] == 0)
    # round 0's footprint is the floor's rectangle: 4 x 4 about (2, 2)
    assert np.allclose(feet.rect[0, :2], (2, 2), atol=0.01) and np.allclose(np.sort(feet.rect[0, 4:]), (2, 2), atol=0.01)
    assert abs(feet.area[0] - 16) < 0.1
    ps = segmentation.PlaneSegmentation(t, DistanceThreshold=0.02, MaxPlanes=mp, MinInliers=600, MaxIterations=n_hyp, Seed=0)
    groups = ps.Extract()
    assert len(groups) == 4 and [len(g) for g in groups] == host.sizes[:4].tolist()  # (Seed 0 draws SC.samples(.., 0))
    assert np.array_equal(np.concatenate(groups), host.ids) and np.array_equal(bits(ps.planes), bits(host.planes[:4]))
    assert np.array_equal(ps.Boxes().obb, geo.obb) and np.array_equal(ps.Footprints().rect, feet.rect)
    ps.SetAxis((0, 0, 1))
    ps.SetEpsAngle(np.radians(10))
    ps.SetMaxPlanes(1)
    floor = ps.Extract()
    assert len(floor) == 1 and ps.planes[0, 2] > 0.999 and abs(len(floor[0]) - 6000) < 360
