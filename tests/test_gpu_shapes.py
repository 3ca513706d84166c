"""Cylinder and sphere segmentation on the GPU (KDTree.Shapes / ShapesDev, csrc/shapes.hip) against the NumPy restatement
of its contract (tests/shape_oracle.py).  Rule of every case: the integer outputs are array_equal to the oracle evaluated
at the library's own hyp_shapes; hyp_shapes and unrefined shapes are equal to the oracle's by uint32 view; a refitted
record lies within the oracle's derived tolerance of the oracle's own refit (exact sums, a float64 solve), its kept axis
and its zeros equal by bits; the padding is checked; a second call gives the first call's bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shape_oracle as SO  # noqa: E402
import shape_scenes as SC  # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
INT_FIELDS = ("n_shapes", "sizes", "refined", "best", "labels", "ids", "status", "counts")
OPTIONAL = ("ids", "status", "counts", "hyp_shapes")
NAMES = dict(max_shapes="MaxShapes", min_inliers="MinInliers", sample_radius="SampleRadius", r_min="RMin", r_max="RMax",
             axis="Axis", min_axis_cos="MinAxisCos", min_normal_cos="MinNormalCos", refine="Refine")


@pytest.fixture(scope="module")
def K():
    from pcgol_amd import kdtree
    return kdtree


@pytest.fixture(scope="module")
def yard(K):
    P, M, part = SC.yard()
    return P, M, part, K.KDTree(P)


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def same(a, b):
    for f in a._fields:
        x, y = getattr(a, f), getattr(b, f)
        assert np.array_equal(bits(x), bits(y)) if np.asarray(x).dtype == f32 else np.array_equal(x, y), f


def lib_args(kw):
    return {NAMES[k]: v for k, v in kw.items()}


def library_range(t, P, radius):
    """a range_of= for the oracle: KDTree.Range's own set about each point of the tree (Range is pinned to the reference
    by its own tests; on a tree that holds non-finite points it is not the brute-force ball)"""
    offs, ids, _ = t.RangeBatch(np.nan_to_num(P, nan=1e30, posinf=1e30, neginf=-1e30), radius)
    return lambda i: ids[offs[i]:offs[i + 1]]


def check(K, t, P, M, kind, smp, max_dist, n_hyp, deleted=None, again=True, range_of=None, **kw):
    """Shapes on the host form against the oracle -> (library result, oracle result)."""
    got = t.Shapes(kind, max_dist, M, NHyp=n_hyp, Samples=smp, **lib_args(kw))
    want = SO.segment(P, M, kind, smp, max_dist, n_hyp, deleted=deleted, hyp_shapes=got.hyp_shapes, lib_shapes=got.shapes,
                      lib_refined=got.refined, range_of=range_of, **kw)
    for f in INT_FIELDS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), (f, getattr(got, f), getattr(want, f))
    assert np.array_equal(bits(got.hyp_shapes), bits(want.hyp_shapes))
    for r in range(len(got.shapes)):
        if got.refined[r]:
            f = want.refits[r]
            print("round %d refit: n %d kappa %.3g tol %.3g, off by %s" % (
                r, f.n, f.kappa, f.tol, np.abs(got.shapes[r, :4].astype(np.float64) - f.rec[:4].astype(np.float64))))
            assert f.ok and np.all(np.abs(got.shapes[r, :4].astype(np.float64) - f.rec[:4].astype(np.float64)) <= f.tol)
            assert np.array_equal(bits(got.shapes[r, 4:]), bits(f.rec[4:]))
        else:
            assert np.array_equal(bits(got.shapes[r]), bits(want.shapes[r]))
    assert got.labels.dtype == np.int64 and len(got.labels) == len(P)
    if again:
        same(got, t.Shapes(kind, max_dist, M, NHyp=n_hyp, Samples=smp, **lib_args(kw)))
    return got, want


def shapes_dev(K, t, M, kind, smp, max_dist, n_hyp, max_shapes=1, want=OPTIONAL, **kw):
    """The device form over torch tensors filled with rubbish -> the same tuple, ids with their padding."""
    import torch
    dev = torch.device("cuda", 0)
    n, rows = t.Len(), max(n_hyp * max_shapes, 1)
    i32 = torch.int32
    d_smp = torch.from_numpy(np.ascontiguousarray(smp, u32).reshape(-1).view(np.int32).copy()).to(dev)
    d_n, d_sz, d_rf, d_bs = (torch.full((k,), -7, dtype=i32, device=dev) for k in (1, max_shapes, max_shapes, max_shapes))
    d_sh = torch.full((max_shapes, 8), 7.0, dtype=torch.float32, device=dev)
    d_lab, d_ids = (torch.full((max(n, 1),), -7, dtype=i32, device=dev) for _ in range(2))
    d_st, d_cn = (torch.full((rows,), -7, dtype=i32, device=dev) for _ in range(2))
    d_hp = torch.full((rows, 8), 7.0, dtype=torch.float32, device=dev)
    d_nrm = torch.from_numpy(np.ascontiguousarray(M, f32)).to(dev)
    opt = dict(ids=d_ids, status=d_st, counts=d_cn, hyp_shapes=d_hp)
    ptr = {k: (v.data_ptr() if k in want else 0) for k, v in opt.items()}
    torch.cuda.synchronize()
    t.ShapesDev(kind, max_dist, d_nrm.data_ptr(), d_smp.data_ptr() if n_hyp else 0, n_hyp, d_n.data_ptr(), d_sh.data_ptr(),
                d_sz.data_ptr(), d_rf.data_ptr(), d_bs.data_ptr(), d_lab.data_ptr(), d_ids=ptr["ids"], d_status=ptr["status"],
                d_counts=ptr["counts"], d_hyp_shapes=ptr["hyp_shapes"], MaxShapes=max_shapes,
                stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    c = lambda x: x.cpu().numpy()  # noqa: E731
    return K.ShapeSegments(int(c(d_n)[0]), c(d_sh), c(d_sz).astype(np.int64), c(d_rf), c(d_bs).astype(np.int64),
                           c(d_lab)[:n].astype(np.int64), c(d_ids)[:n].astype(np.int64), c(d_st)[:n_hyp * max_shapes],
                           c(d_cn)[:n_hyp * max_shapes].astype(np.int64), c(d_hp)[:n_hyp * max_shapes])


def same_as_host(dev, host, n):
    k = len(host.ids)
    assert np.array_equal(dev.ids[:k], host.ids) and np.all(dev.ids[k:] == -1) and len(dev.ids) == n  # the padding
    assert dev.n_shapes == host.n_shapes
    for f in ("sizes", "refined", "best", "labels"):
        assert np.array_equal(getattr(dev, f), getattr(host, f)), f
    assert np.array_equal(dev.status, host.status.reshape(-1)) and np.array_equal(dev.counts, host.counts.reshape(-1))
    assert np.array_equal(bits(dev.shapes), bits(host.shapes))
    assert np.array_equal(bits(dev.hyp_shapes), bits(host.hyp_shapes.reshape(-1, 8)))


def groups_of(r):
    return np.split(r.ids, np.cumsum(r.sizes[:r.n_shapes])[:-1])


@pytest.mark.parametrize("n_hyp", [128, 256])
@pytest.mark.parametrize("call", sorted(SC.CALLS))
def test_yard_peels_its_shapes_and_stops(K, yard, call, n_hyp):
    P, M, part, t = yard
    kind, kw, holds = SC.CALLS[call]
    smp = SC.samples(n_hyp, 5, SC.SEEDS[0])
    for refine in (False, True):
        got, want = check(K, t, P, M, kind, smp, n_hyp=n_hyp, max_shapes=5, refine=refine, **SC.YARD, **kw)
        m = len(holds)
        assert got.n_shapes == m and np.all(got.status[m] >= 0) and np.all(got.status[m + 1:] == -1)
        assert np.all(got.counts[m + 1:] == 0) and np.all(got.hyp_shapes[m + 1:] == 0) and got.counts[m].max() < 550
        assert np.all(got.sizes[m:] == 0) and np.all(got.best[m:] == -1) and np.all(got.shapes[m:] == 0)
        assert np.all(got.refined[m:] == 0) and (refine or not got.refined.any())
        found = [int(np.bincount(part[g], minlength=6).argmax()) for g in groups_of(got)]
        assert sorted(found) == sorted(holds)
        radius = {SC.POLE_A: 0.10, SC.POLE_B: 0.15, SC.PIPE: 0.08, SC.BALL: 0.3}
        for r, k in enumerate(found):
            assert abs(got.shapes[r, 3] - radius[k]) < 0.02 and got.sizes[r] > 800
        if refine:
            assert got.refined[:m].all()  # (the oracle test: on this scene every refit loses no inlier)


def test_yard_every_split_both_forms_and_null_outputs(K, yard, monkeypatch):
    P, M, part, t = yard
    n_hyp = 128
    kind, kw, holds = SC.CALLS["cylinders"]
    smp = SC.samples(n_hyp, 5, SC.SEEDS[0])
    args = lib_args(dict(min_inliers=600, min_normal_cos=0.8, **kw))
    monkeypatch.delenv("PCGX_SHAPES_SPLIT", raising=False)
    host = t.Shapes(kind, 0.02, M, NHyp=n_hyp, MaxShapes=5, Samples=smp, **args)
    assert host.n_shapes == 3
    for s in (1, 3, len(P) + 5):
        monkeypatch.setenv("PCGX_SHAPES_SPLIT", str(s))
        same(host, t.Shapes(kind, 0.02, M, NHyp=n_hyp, MaxShapes=5, Samples=smp, **args))
    same_as_host(shapes_dev(K, t, M, kind, smp, 0.02, n_hyp, max_shapes=5, **args), host, len(P))
    monkeypatch.delenv("PCGX_SHAPES_SPLIT")
    same_as_host(shapes_dev(K, t, M, kind, smp, 0.02, n_hyp, max_shapes=5, **args), host, len(P))
    for leave in OPTIONAL:  # each optional output NULL: the others do not change
        d = shapes_dev(K, t, M, kind, smp, 0.02, n_hyp, max_shapes=5, want=tuple(k for k in OPTIONAL if k != leave), **args)
        assert np.all(np.asarray(getattr(d, leave)).reshape(-1) == (7 if leave == "hyp_shapes" else -7))  # untouched
        assert d.n_shapes == 3 and np.array_equal(d.labels, host.labels) and np.array_equal(bits(d.shapes), bits(host.shapes))
        if leave != "ids":
            assert np.array_equal(d.ids[:len(host.ids)], host.ids)
    # the spheres, without the normal test (the other two count kernels), in both forms
    kind, kw, holds = SC.CALLS["spheres"]
    got, _ = check(K, t, P, M, kind, smp[:2], 0.02, n_hyp, max_shapes=2, min_inliers=600, **kw)
    same_as_host(shapes_dev(K, t, M, kind, smp[:2], 0.02, n_hyp, max_shapes=2, **lib_args(dict(min_inliers=600, **kw))), got,
                 len(P))
    kind, kw, holds = SC.CALLS["poles"]
    check(K, t, P, M, kind, smp[:2], 0.02, n_hyp, max_shapes=2, min_inliers=600, **kw)


def test_yard_on_the_walk_and_on_a_patched_tree(K, yard, monkeypatch):
    P, M, part, t = yard
    n_hyp = 128
    smp = SC.samples(n_hyp, 4, SC.SEEDS[0])
    for call in ("cylinders", "spheres"):
        kind, kw, holds = SC.CALLS[call]
        monkeypatch.delenv("PCGX_RANGE_WALK", raising=False)
        grid, _ = check(K, t, P, M, kind, smp, n_hyp=n_hyp, max_shapes=4, **SC.YARD, **kw)
        monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        walk, _ = check(K, t, P, M, kind, smp, n_hyp=n_hyp, max_shapes=4, **SC.YARD, **kw)
        same(grid, walk)  # the partner is a property of the set: the same bits on both enumerations
        monkeypatch.delenv("PCGX_RANGE_WALK")
    # a handle with a tenth of its ids deleted walks the patched tree: never seeds, partners or inliers
    td = K.KDTree(P)
    gone = np.random.default_rng(2).permutation(len(P))[:len(P) // 10]
    td.DeletePoints(gone)
    deleted = np.zeros(len(P), bool)
    deleted[gone] = True
    kind, kw, holds = SC.CALLS["cylinders"]
    yd = dict(SC.YARD, min_inliers=540)
    got, want = check(K, td, P, M, kind, smp, n_hyp=n_hyp, max_shapes=4, deleted=deleted, **yd, **kw)
    assert got.n_shapes == 3 and np.all(got.labels[gone] == -1) and not np.isin(got.ids, gone).any()
    assert not np.isin(want.partners, gone).any() and (want.partners >= 0).sum() > n_hyp
    args = lib_args({k: v for k, v in dict(yd, **kw).items() if k != "max_dist"})
    same_as_host(shapes_dev(K, td, M, kind, smp, 0.02, n_hyp, max_shapes=4, **args), got, len(P))


def test_global_partner(K, yard):
    P, M, part, t = yard
    n_hyp = 256
    smp = SC.samples(n_hyp, 2, 3)
    # the partner out of everything that is left: two points on the ball once in 75 draws
    got, want = check(K, t, P, M, SO.SPHERE, smp, 0.02, n_hyp, max_shapes=2, min_inliers=600, min_normal_cos=0.8, r_min=0.1,
                      r_max=0.6)
    assert np.array_equal(want.partners[0] < 0, got.status[0] == SO.NO_PARTNER)
    # the same word twice: i1 == i0, status 1 on every row, nothing found, the next round does not run
    twice = np.repeat(smp[:, :, :1], 2, axis=2)
    got, _ = check(K, t, P, M, SO.SPHERE, twice, 0.02, n_hyp, max_shapes=2)
    assert np.all(got.status[0] == SO.NO_PARTNER) and np.all(got.status[1] == -1) and got.n_shapes == 0
    assert np.all(got.counts == 0) and np.all(got.hyp_shapes == 0) and got.best.tolist() == [-1, -1]
    mixed = smp.copy()
    mixed[0, ::2, 1] = mixed[0, ::2, 0]
    got, _ = check(K, t, P, M, SO.CYLINDER, mixed[:1], 0.02, n_hyp, max_shapes=1, r_max=1.0)
    assert np.all(got.status[0, ::2] == SO.NO_PARTNER) and (got.status[0, 1::2] != SO.NO_PARTNER).all()


def test_fat_row_partner(K, monkeypatch):
    """one site taken 4200 times inside the seeds' radius: on the grid the row is shared by the wave, the partial minima
    reduced into the owner; the partner is the oracle's on the grid, the walk and the patched walk alike"""
    from pcgol_amd import _lib as L
    P, M = SC.fat_site()
    monkeypatch.setenv("PCGX_GRID", "2")  # (a grid even with a crowded cell)
    t = K.KDTree(P)
    st = (C.c_int64 * 14)()
    L.check(L.lib().pcgx_debug_grid_stats(t._h, None, 0, 1.0, st))
    assert st[3] == 1, list(st)
    heap = np.flatnonzero(np.all(P == P[np.flatnonzero(np.all(P == f32([0.0, 0.6, 0.8]), axis=1))[0]], axis=1))
    assert len(heap) == 4200
    n_hyp = 200
    smp = SC.samples(n_hyp, 2, 9)
    R = len(P)
    sparse = np.setdiff1d(np.arange(R), heap)
    smp[0, :100, 0] = [SC.word_for(int(i), R) for i in sparse[:100]]  # half the seeds off the heap, some beside it
    kw = dict(max_shapes=2, sample_radius=0.5, r_min=0.5, r_max=2.0, min_inliers=50)
    got, want = check(K, t, P, M, SO.SPHERE, smp, 0.02, n_hyp, **kw)
    near = SO.range_set(P[sparse[:100]], P[heap[0]], 0.5)
    assert near.sum() >= 5 and np.isin(want.partners[0, :100][near], heap).any()  # a fat row was some seed's partner's
    assert np.isin(want.partners[0, 100:], heap).sum() > 50 and got.n_shapes >= 1
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    walk, _ = check(K, t, P, M, SO.SPHERE, smp, 0.02, n_hyp, again=False, **kw)
    same(got, walk)
    monkeypatch.delenv("PCGX_RANGE_WALK")
    gone = np.concatenate([heap[:7], sparse[100:130]])
    t.DeletePoints(gone)
    deleted = np.zeros(R, bool)
    deleted[gone] = True
    got, want = check(K, t, P, M, SO.SPHERE, smp, 0.02, n_hyp, deleted=deleted, again=False, **kw)
    assert not np.isin(want.partners, gone).any()


def test_launch_boundaries(K):
    tile = K.ShapesTile()
    assert tile == 128
    P, M, part = SC.yard()
    keep = np.flatnonzero(part == SC.BALL)[:700]
    Pb, Mb = P[keep], M[keep]
    tb = K.KDTree(Pb)
    for n_hyp in (1, tile - 1, tile, tile + 1, 2 * tile + 1):
        got, _ = check(K, tb, Pb, Mb, SO.SPHERE, SC.samples(n_hyp, 2, n_hyp), 0.02, n_hyp, max_shapes=2, min_inliers=50,
                       sample_radius=0.4, r_min=0.1, r_max=0.6, min_normal_cos=0.8)
        assert n_hyp < 64 or got.n_shapes >= 1
    rng = np.random.default_rng(4)
    for n in (1, 2, 63, 64, 65, 257, 1024, 1025):
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        Q, N = (d * 0.5).astype(f32), d.astype(f32)
        for kind in (SO.SPHERE, SO.CYLINDER):
            got, _ = check(K, K.KDTree(Q), Q, N, kind, SC.samples(40, 3, n), 0.02, 40, max_shapes=3, sample_radius=0.6,
                           again=kind == SO.SPHERE)
            if n < 2:
                assert got.n_shapes == 0 and np.all(got.status == -1) and np.all(got.labels == -1)
            elif kind == SO.SPHERE and n >= 63:
                assert got.n_shapes >= 1 and got.sizes[0] >= n - 2 and abs(got.shapes[0, 3] - 0.5) < 0.01
            if n == 2 and got.n_shapes == 1:
                assert got.sizes.tolist() == [2, 0, 0] and np.all(got.status[1:] == -1)  # R_1 = 0: the round cannot run


def test_edges_of_the_contract(K):
    rng = np.random.default_rng(7)
    n_hyp = 40
    smp = SC.samples(n_hyp, 6, 15)
    nanc = np.full((100, 3), np.nan, f32)
    ones = np.tile(f32([0, 0, 1]), (100, 1))
    got, _ = check(K, K.KDTree(nanc), nanc, ones, SO.SPHERE, smp[:2], 0.02, n_hyp, max_shapes=2, sample_radius=0.5)
    assert got.n_shapes == 0 and np.all(got.status == -1) and np.all(got.labels == -1) and len(got.ids) == 0
    d = rng.normal(size=(600, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    Q, N = d.astype(f32), d.astype(f32)
    Q[::5, 0] = np.inf
    Q[1::5, 2] = np.nan
    Q[2::50] = -np.inf
    N[3::5] = 0
    N[4::25, 1] = np.nan
    N[9::25, 0] = np.inf
    live = SO.live_mask(Q, N)
    t = K.KDTree(Q)
    near = library_range(t, Q, 0.7)  # (the seeds are live points: their Range is asked at their own coordinates)
    for kind in (SO.SPHERE, SO.CYLINDER):
        for max_shapes in (1, 6):
            got, _ = check(K, t, Q, N, kind, smp[:max_shapes], 0.02, n_hyp, max_shapes=max_shapes, sample_radius=0.7,
                           min_normal_cos=0.9, range_of=near)
            assert np.all(got.labels[~live] == -1) and got.n_shapes >= 1
        assert kind == SO.CYLINDER or got.sizes[0] == live.sum()
    # a seed with an empty neighbourhood: status 1; a radius window nothing passes: status 4, nothing found
    got, _ = check(K, t, Q, N, SO.SPHERE, smp[:2], 0.02, n_hyp, max_shapes=2, sample_radius=1e-4)
    assert np.all(got.status[0] == SO.NO_PARTNER) and got.n_shapes == 0 and np.all(got.status[1] == -1)
    got, _ = check(K, t, Q, N, SO.SPHERE, smp[:2], 0.02, n_hyp, max_shapes=2, sample_radius=0.7, r_min=5.0, r_max=np.inf,
                   range_of=near)
    assert set(got.status[0].tolist()) <= {SO.DEGENERATE, SO.RADIUS} and got.n_shapes == 0 and got.best.tolist() == [-1, -1]
    t.DeletePoints(np.arange(len(Q)))  # every point deleted
    got, _ = check(K, t, Q, N, SO.SPHERE, smp[:2], 0.02, n_hyp, max_shapes=2, sample_radius=0.7,
                   deleted=np.ones(len(Q), bool))
    assert got.n_shapes == 0 and np.all(got.status == -1)
    # n_hyp == 0 is fine and finds nothing, on both forms
    t = K.KDTree(Q)
    got = t.Shapes(SO.SPHERE, 0.02, N, NHyp=0, MaxShapes=3)
    assert got.n_shapes == 0 and np.all(got.labels == -1) and got.best.tolist() == [-1] * 3 and got.status.shape == (3, 0)
    dv = shapes_dev(K, t, N, SO.SPHERE, smp, 0.02, 0, max_shapes=3)
    assert dv.n_shapes == 0 and np.all(dv.labels == -1) and np.all(dv.ids == -1) and dv.best.tolist() == [-1] * 3
    assert np.all(dv.sizes == 0) and np.all(dv.shapes == 0) and np.all(dv.refined == 0)


def test_refinement_rules(K):
    for kind in (SO.SPHERE, SO.CYLINDER):
        P, M, w = SC.refit_loses(kind)
        t = K.KDTree(P)
        off, _ = check(K, t, P, M, kind, w, 0.02, 1, refine=False)
        on, want = check(K, t, P, M, kind, w, 0.02, 1, refine=True)
        assert want.refits[0].ok  # the refit loses the low point: the hypothesis is kept
        assert on.refined.tolist() == [0] and on.sizes.tolist() == [13] and np.array_equal(bits(on.shapes), bits(off.shapes))
        Q, M, w = SC.refit_loses(kind, low=1.019)
        on, want = check(K, K.KDTree(Q), Q, M, kind, w, 0.02, 1, refine=True)
        assert on.refined.tolist() == [1] and on.sizes.tolist() == [13] and 1.01 < on.shapes[0, 3] < 1.019
        # no refit: the radius window holds the hypothesis's 1 and not the refit's 1.016
        on, want = check(K, K.KDTree(Q), Q, M, kind, w, 0.02, 1, refine=True, r_max=1.0)
        assert on.refined.tolist() == [0] and not want.refits[0].ok and on.shapes[0, 3] == 1.0


def test_invalid_arguments_write_nothing(K, yard):
    from pcgol_amd import _lib as L
    P, M, part, t = yard
    smp = SC.samples(8, 2, 1)
    nan, inf = float("nan"), float("inf")
    bad = [dict(Kind=2), dict(Kind=-1), dict(NHyp=-1), dict(MaxShapes=0), dict(MaxShapes=257), dict(MaxDist=0.0),
           dict(MaxDist=-1.0), dict(MaxDist=inf), dict(MaxDist=nan), dict(MinInliers=-1), dict(Axis=(0, 0, 0)),
           dict(Axis=(0, nan, 1)), dict(Axis=(np.inf, 0, 1)), dict(Axis=(0, 0, 1), MinAxisCos=1.5),
           dict(Axis=(0, 0, 1), MinAxisCos=-0.1), dict(Axis=(0, 0, 1), MinAxisCos=nan), dict(MinNormalCos=1.01),
           dict(MinNormalCos=-0.5), dict(MinNormalCos=nan), dict(SampleRadius=-0.1), dict(SampleRadius=inf),
           dict(SampleRadius=nan), dict(RMin=nan), dict(RMax=nan), dict(RMin=-1.0), dict(RMax=-1.0), dict(RMin=2.0, RMax=1.0),
           dict(RMin=inf, RMax=1.0), dict(Normals=None)]
    for kw in bad:
        a = dict(Kind=1, MaxDist=0.02, Normals=M, NHyp=8, MaxShapes=2, Samples=smp)
        a.update(kw)
        with pytest.raises((L.PcgxError, ValueError)):
            t.Shapes(a.pop("Kind"), a.pop("MaxDist"), a.pop("Normals"), **a)
    # an unused bound is not checked (no axis); r_max may be +inf, r_min == r_max is a window
    assert t.Shapes(1, 0.02, M, NHyp=8, MaxShapes=2, Samples=smp, MinAxisCos=7.0, RMin=0.1, RMax=inf).n_shapes >= 0
    assert t.Shapes(0, 0.02, M, NHyp=8, MaxShapes=2, Samples=smp, RMin=0.3, RMax=0.3).n_shapes >= 0
    # ... and nothing is written: the raw call with rubbish in every output
    n = len(P)
    out = [np.full(k, 77, d) for k, d in ((16, f32), (2, np.int64), (2, np.int32), (2, np.int64), (n, np.int64), (n, np.int64),
                                          (16, np.int32), (16, np.int64), (128, f32))]
    cnt = C.c_int64(77)
    lib = L.lib()

    def raw(tree=t._h, kind=1, samples=L.ptr(smp), n_hyp=8, mp=2, md=0.02, sr=0.3, r_min=0.0, r_max=1.0, normals=L.ptr(M),
            skip=None):
        ptrs = [None if i == skip else L.ptr(a) for i, a in enumerate(out)]
        return lib.pcgx_kdtree_shapes(tree, kind, samples, n_hyp, mp, md, 3, sr, r_min, r_max, None, 0.0, normals, 0.0, 1,
                                      C.byref(cnt), *ptrs)
    calls = [dict(tree=None), dict(kind=5), dict(samples=None), dict(mp=300), dict(md=nan), dict(n_hyp=-2), dict(sr=-1.0),
             dict(r_min=2.0), dict(r_max=nan), dict(normals=None), dict(n_hyp=2 ** 24, mp=256)] + [dict(skip=i) for i in range(5)]
    for kw in calls:
        assert raw(**kw) == L.PCGX_E_INVALID, kw
        assert cnt.value == 77 and all(np.all(a == 77) for a in out), kw
    assert raw(skip=5) == L.PCGX_OK and np.all(out[5] == 77) and cnt.value != 77  # ids may be NULL


def test_segmentation_feeds_group_geometry(K, yard):
    """ShapeSegmentation's Extract, Boxes and Footprints on the yard, and ShapesDev -> GroupStatsDev -> GroupHullsDev on
    one stream with no synchronise in between: equal to the host forms."""
    import torch
    from pcgol_amd import segmentation
    P, M, part, t = yard
    n, n_hyp, mp = len(P), 128, 4
    kind, kw, holds = SC.CALLS["poles"]
    ss = segmentation.ShapeSegmentation(t, M, Model="cylinder", DistanceThreshold=0.02, MaxShapes=mp, MinInliers=600,
                                        MaxIterations=n_hyp, SampleRadius=0.3, RadiusLimits=(0.03, 0.3), NormalMinCos=0.8,
                                        Seed=SC.SEEDS[0])
    ss.SetAxis((0, 0, 1))
    ss.SetEpsAngle(float(np.arccos(0.95)))
    groups = ss.Extract()
    smp = SC.samples(n_hyp, mp, SC.SEEDS[0])  # (Seed s draws SC.samples(.., s))
    args = lib_args(dict(min_inliers=600, min_normal_cos=0.8, **kw))
    args["MinAxisCos"] = ss.min_axis_cos
    host = t.Shapes(kind, 0.02, M, NHyp=n_hyp, MaxShapes=mp, Samples=smp, **args)
    assert len(groups) == host.n_shapes == 2 and [len(g) for g in groups] == host.sizes[:2].tolist()
    assert np.array_equal(np.concatenate(groups), host.ids) and np.array_equal(bits(ss.shapes), bits(host.shapes[:2]))
    geo, feet = t.GroupStats(host.ids, host.sizes[:2]), t.GroupHulls(host.ids, host.sizes[:2])
    assert np.array_equal(ss.Boxes().obb, geo.obb) and np.array_equal(ss.Footprints().rect, feet.rect)
    # an upright pole's footprint is a square of its diameter about where the scene put it (the record's own q may lie a
    # centimetre off: the hypothesis's axis leans a little and is not refitted)
    for r in range(2):
        x, y, rad = (4.0, 2.0, 0.15) if host.shapes[r, 3] > 0.125 else (1.5, 1.5, 0.10)
        assert np.allclose(feet.rect[r, :2], (x, y), atol=0.01) and np.allclose(feet.rect[r, 4:], rad, atol=0.025)
        assert np.allclose(host.shapes[r, :2], (x, y), atol=0.05) and abs(host.shapes[r, 3] - rad) < 0.01
    dev = torch.device("cuda", 0)
    i32, f64 = torch.int32, torch.float64
    d_smp = torch.from_numpy(smp.reshape(-1).view(np.int32).copy()).to(dev)
    d_nrm = torch.from_numpy(M).to(dev)
    d_n, d_sz, d_rf, d_bs = (torch.full((k,), -7, dtype=i32, device=dev) for k in (1, mp, mp, mp))
    d_sh = torch.zeros((mp, 8), dtype=torch.float32, device=dev)
    d_lab, d_ids, h_ids = (torch.full((n,), -7, dtype=i32, device=dev) for _ in range(3))
    g_cnt, h_sz = (torch.zeros(mp, dtype=i32, device=dev) for _ in range(2))
    g_obb, h_rect = (torch.zeros((mp, 6), dtype=f64, device=dev) for _ in range(2))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t.ShapesDev(kind, 0.02, d_nrm.data_ptr(), d_smp.data_ptr(), n_hyp, d_n.data_ptr(), d_sh.data_ptr(), d_sz.data_ptr(),
                    d_rf.data_ptr(), d_bs.data_ptr(), d_lab.data_ptr(), d_ids=d_ids.data_ptr(), MaxShapes=mp,
                    stream=s.cuda_stream, **args)
        t.GroupStatsDev(d_ids.data_ptr(), n, d_sz.data_ptr(), mp, d_n_groups=d_n.data_ptr(), d_count=g_cnt.data_ptr(),
                        d_obb=g_obb.data_ptr(), stream=s.cuda_stream)
        t.GroupHullsDev(d_ids.data_ptr(), n, d_sz.data_ptr(), mp, d_n_groups=d_n.data_ptr(), d_hull_sizes=h_sz.data_ptr(),
                        d_hull_ids=h_ids.data_ptr(), d_rect=h_rect.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert int(d_n[0]) == 2 and np.array_equal(d_lab.cpu().numpy(), host.labels)
    assert np.array_equal(g_cnt.cpu().numpy()[:2], geo.count) and np.array_equal(g_obb.cpu().numpy()[:2], geo.obb)
    assert np.array_equal(h_rect.cpu().numpy()[:2], feet.rect) and np.all(g_cnt.cpu().numpy()[2:] == 0)
