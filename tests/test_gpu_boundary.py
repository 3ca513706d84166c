"""GPU: boundary points over radius neighbourhoods (csrc/boundary.hip, csrc/boundary_terms.h) against
tests/boundary_oracle.py.  Every output is an OR or an integer sum over a point set, so masks, gaps, counts and ids are
compared with array_equal on every kind of handle: the grid, the forced walk and a handle after DeletePoints."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import features, kdtree, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_oracle as BO  # noqa: E402
import boundary_scenes as BS  # noqa: E402
import normals_oracle as NO  # noqa: E402
from test_gpu_radius_edges import HEAPS, _assert_heap_grid, _grid_on, _heap_scene, _range_count  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64, u64 = np.float32, np.float64, np.uint64
nan, inf = np.nan, np.inf

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _raw(t, r, nrm, min_gap=16, min_nb=1):
    """the host entry point's whole output: ids [Len()], n_ids, gaps, masks, counts"""
    n = t.Len()
    nrm = np.ascontiguousarray(nrm, f32).reshape(-1, 3)
    assert len(nrm) == n
    ids, gaps = np.full(n, -7, np.int64), np.full(n, -7, np.int32)
    masks, counts = np.full(n, 0x5555, u64), np.full(n, -7, np.int32)
    cnt = C.c_int64(-7)
    L.check(L.lib().pcgx_kdtree_boundary(t._h, float(r), L.ptr(nrm), int(min_gap), int(min_nb), L.ptr(ids), C.byref(cnt),
                                         L.ptr(gaps), L.ptr(masks), L.ptr(counts)))
    return ids, cnt.value, gaps, masks, counts


def _boundary(t, r, nrm, min_gap=16, min_nb=1, what=""):
    """Boundary with the output convention checked (ascending ids, then -1 in every remaining slot) and the same bits
    from a second call -> (ids, gaps, masks, counts)"""
    ids, m, gaps, masks, counts = _raw(t, r, nrm, min_gap, min_nb)
    assert 0 <= m <= len(ids) and np.all(ids[m:] == -1) and np.all(np.diff(ids[:m]) > 0) and np.all(ids[:m] >= 0), what
    again = _raw(t, r, nrm, min_gap, min_nb)
    assert again[1] == m and all(np.array_equal(a, b) for a, b in zip((ids, gaps, masks, counts),
                                                                      (again[0],) + again[2:])), what
    return ids[:m], gaps, masks, counts


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


# ------------------------------------------------------------------------------------------------ 1. the lattice

def test_lattice():
    pts, kind = BS.lattice()
    t = kdtree.New(pts)
    want_gaps = np.array([BS.LATTICE_GAPS[k] for k in ("interior", "edge", "corner")])[kind]
    for nz in (1.0, -1.0):
        nrm = np.tile(f32([0, 0, nz]), (len(pts), 1))
        ids, gaps, masks, counts = _boundary(t, BS.LATTICE_RADIUS, nrm, 16)
        assert np.array_equal(gaps, want_gaps)
        assert np.array_equal(ids, np.nonzero(kind > 0)[0]) and len(ids) == 24
        assert np.array_equal(counts, np.array([9, 6, 4])[kind])
        BO.check(BO.boundary(pts, nrm, BS.LATTICE_RADIUS, 16), ids, gaps, masks, counts, nz)
        ids32 = _boundary(t, BS.LATTICE_RADIUS, nrm, 32)[0]
        assert np.array_equal(ids32, np.nonzero(kind == 2)[0]) and len(ids32) == 4


# ------------------------------------------------------------------------------------------------ 2. the plate

def _plate():
    def make():
        pts = BS.plate()
        t = kdtree.New(pts)
        nrm = t.Normals(BS.PLATE_RADIUS, Viewpoint=(40.0, 40.0, 500.0))[0]
        lists = NO.brute_force_lists(pts, pts, BS.PLATE_RADIUS)
        return pts, t, nrm, lists
    return _cached("plate", make)


def test_plate_with_holes_on_every_handle(monkeypatch):
    pts, t, nrm, (offs, nbr) = _plate()
    r, n = BS.PLATE_RADIUS, len(pts)
    assert BO.usable(nrm).all() and len(np.unique(nrm, axis=0)) > n // 2  # the library's normals, and they vary
    ref = BO.from_lists(pts, nrm, offs, nbr, BS.PLATE_MIN_GAP)
    # what the scene is for, by the oracle alone
    d = BS.rim_distance(pts)
    flagged = np.zeros(n, bool)
    flagged[ref["ids"]] = True
    assert 0.04 < flagged.mean() < 0.10
    assert not np.any(flagged & (d > r))
    assert (d < 0.5).sum() > 300 and np.all(flagged[d < 0.5])
    assert _grid_on(t)[3] == 1
    got = _boundary(t, r, nrm, BS.PLATE_MIN_GAP, what="grid")
    BO.check(ref, *got, what="grid")
    assert np.array_equal(got[3].astype(np.int64), _range_count(t, pts, r))
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    walk = _boundary(t, r, nrm, BS.PLATE_MIN_GAP, what="walk")
    BO.check(ref, *walk, what="walk")
    assert np.array_equal(walk[3].astype(np.int64), _range_count(t, pts, r))
    monkeypatch.delenv("PCGX_RANGE_WALK")
    gone = np.sort(np.random.default_rng(5).choice(n, n // 10, replace=False))
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    refd = BO.boundary(pts, nrm, r, BS.PLATE_MIN_GAP, deleted=gone)
    gotd = _boundary(td, r, nrm, BS.PLATE_MIN_GAP, what="deleted")
    BO.check(refd, *gotd, what="deleted")
    live = np.setdiff1d(np.arange(n), gone)
    assert np.array_equal(gotd[3][live].astype(np.int64), _range_count(td, pts[live], r)) and not gotd[3][gone].any()
    assert not np.isin(gotd[0], gone).any() and np.all(gotd[1][gone] == -1)
    assert len(np.setdiff1d(gotd[0], got[0])) > 0 and not np.array_equal(gotd[2], got[2])  # the two results differ


# ------------------------------------------------------------------------------------------------ 3. fat rows

HEAP_BALL = 2.0 ** -10  # the radius of a jittered heap: far below the radii, and (asserted) inside one grid row


def _heap_cloud():
    """test_gpu_radius_edges' heap scene with every heap jittered inside a ball of HEAP_BALL, and behind it four
    background points in the heaps' own grid rows, at 1.0 from the centres of the first two heaps and 0.75 from the
    others'.  -> (points, the heaps' ids)"""
    pts = _heap_scene()
    heaps = [np.nonzero(np.all(pts == h, axis=1))[0] for h, _ in HEAPS]
    assert [len(h) for h in heaps] == [m for _, m in HEAPS]
    rng = np.random.default_rng(404)
    for ids in heaps:
        v = rng.standard_normal((len(ids), 3))
        v *= (HEAP_BALL * rng.random(len(ids)) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
        pts[ids] = (pts[ids].astype(f64) + v).astype(f32)
    extra = [h + f32([1.0, 0, 0]) for h, _ in HEAPS[:2]] + [h - f32([0.75, 0, 0]) for h, _ in HEAPS[2:]]
    return np.ascontiguousarray(np.concatenate([pts, np.array(extra, f32)]), f32), heaps


def _assert_heaps_in_one_row(t, pts, heaps):
    """every heap lies in one (y, z) row of the grid, so its records are one fat row (the 4095 one: a lane's own)"""
    geom, dims = np.zeros(5, f32), np.zeros(3, np.int32)
    L.check(L.lib().pcgx_debug_grid_geometry(t._h, L.ptr(geom), L.ptr(dims)))
    for ids in heaps:
        for a in (1, 2):
            cell = np.clip((pts[ids, a] - geom[a]) * geom[4], f32(0), f32(dims[a] - 1)).astype(np.int32)
            assert cell.min() == cell.max(), (a, cell.min(), cell.max())


def _heap_case():
    def make():
        pts, heaps = _heap_cloud()
        n = len(pts)
        assert n % 64 != 0  # a partial last wave
        up = pts[:, 2] > 5.0  # the heaps, the sparse points round them, the four extras
        assert pts[up, 2].min() - pts[~up, 2].max() > 1.0  # the slab is nobody's neighbour up there
        rng = np.random.default_rng(405)
        # Unit normals for the points round the heaps and for every eighth heap member; zero normals elsewhere: a point
        # without a frame is not evaluated and enumerates nothing, which keeps the brute force affordable (a heap
        # member's list is its whole heap).
        pick = up.copy()
        for ids in heaps:
            pick[ids] = rng.random(len(ids)) < 0.125
        nrm = np.zeros((n, 3), f32)
        nrm[pick] = _unit(rng, int(pick.sum()))
        return pts, heaps, nrm, np.nonzero(pick)[0], np.nonzero(up)[0]
    return _cached("heap case", make)


def _heap_sectors(r):
    def make():
        pts, heaps, nrm, sel, up = _heap_case()
        offs, nbr = NO.brute_force_lists(pts[up], pts[sel], r)
        nbr = up[nbr]
        return offs, nbr, BO.pair_sectors(pts, nrm, offs, nbr, sel)
    return _cached(("heap sectors", r), make)


@pytest.mark.parametrize("r", [1.0, 0.75])
def test_fat_rows(r, monkeypatch):
    """heaps of 4095, 4096, 4097 and 6000 points inside tiny balls: fat grid rows scanned by whole waves beside a lane's
    own rows -- the wave-wide OR and add and the owner's merge -- on the grid (PCGX_GRID=2), the walk and after
    DeletePoints.  A heap's members see each other in every direction; a background point sees a whole heap in a sector
    or two."""
    pts, heaps, nrm, sel, up = _heap_case()
    n = len(pts)
    offs, nbr, sectors = _heap_sectors(r)
    ref = BO.from_sectors(nrm, offs, nbr, sectors, 16, 1, sel)
    gone = np.unique(np.concatenate([np.random.default_rng(9).choice(n - 4, n // 50, replace=False),
                                     [h[0] for h in heaps[:2]]]))
    refd = BO.from_sectors(nrm, offs, nbr, sectors, 16, 1, sel, deleted=gone)
    # what the scene is for, by the oracle alone
    for h in heaps:
        ev = h[ref["evaluated"][h]]
        assert len(ev) > 400 and np.all(ref["counts"][ev] >= len(h)) and np.median(ref["gaps"][ev]) <= 2
    seen = ref["evaluated"].copy()
    seen[np.concatenate(heaps)] = False
    seen &= ref["counts"] > 4000  # a background point with a heap in its neighbourhood
    assert seen.sum() > 20
    monkeypatch.setenv("PCGX_GRID", "2")
    t = kdtree.New(pts)
    _assert_heap_grid(t)
    _assert_heaps_in_one_row(t, pts, heaps)
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    BO.check(ref, *_boundary(t, r, nrm, what="grid"), what=("grid", r))
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    BO.check(ref, *_boundary(t, r, nrm, what="walk"), what=("walk", r))
    monkeypatch.delenv("PCGX_RANGE_WALK")
    gotd = _boundary(td, r, nrm, what="deleted")
    BO.check(refd, *gotd, what=("deleted", r))
    assert not np.isin(gotd[0], gone).any() and not np.array_equal(refd["counts"], ref["counts"])


# ------------------------------------------------------------------------------------------------ 4. the device chain

def test_device_chain():
    """NormalsDev -> BoundaryDev on one torch stream, nothing copied in between: the host entry point's bits; again with
    every optional output left out; two calls give the same bits"""
    import torch
    dev = torch.device("cuda", 0)
    pts = synth.surface_cloud(20_000, 5.0, 33)[0]
    t = kdtree.New(pts)
    n, r, vp = len(pts), 0.12, (0.3, -2.0, 25.0)
    nrm = t.Normals(r, Viewpoint=vp)[0]
    want = t.Boundary(r, nrm)
    assert 0 < len(want[0]) < n

    def outs():
        return (torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((1,), -7, dtype=torch.int32, device=dev))
    dn = torch.empty((n, 3), dtype=torch.float32, device=dev)
    (di, dc), (di2, dc2), (di3, dc3) = outs(), outs(), outs()
    dg, dk = outs()[0], outs()[0]
    dm = torch.full((n,), 0x5555, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        t.NormalsDev(r, dn.data_ptr(), Viewpoint=vp, stream=st)
        t.BoundaryDev(r, dn.data_ptr(), di.data_ptr(), dc.data_ptr(), dg.data_ptr(), dm.data_ptr(), dk.data_ptr(), stream=st)
        t.BoundaryDev(r, dn.data_ptr(), di2.data_ptr(), dc2.data_ptr(), stream=st)  # (no optional outputs)
        t.BoundaryDev(r, dn.data_ptr(), di3.data_ptr(), dc3.data_ptr(), dg.data_ptr(), dm.data_ptr(), dk.data_ptr(), stream=st)
        stream.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(dn.cpu().numpy().view(np.uint32), nrm.view(np.uint32))
    m = int(dc.cpu()[0])
    got = di.cpu().numpy()
    assert m == len(want[0]) and np.array_equal(got[:m], want[0]) and np.all(got[m:] == -1)
    assert np.array_equal(dg.cpu().numpy(), want[1])
    assert np.array_equal(dm.cpu().numpy().view(u64), want[2])
    assert np.array_equal(dk.cpu().numpy(), want[3])
    for c, i in ((dc2, di2), (dc3, di3)):
        assert int(c.cpu()[0]) == m and np.array_equal(i.cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------ 5. the contract's edges

def test_small_lengths():
    for n in range(1, 66):
        rng = np.random.default_rng(500 + n)
        pts = (rng.integers(0, 8, (n, 3)) / 8.0).astype(f32)
        nrm = _unit(rng, n)
        t = kdtree.New(pts)
        for r, g in ((0.3, 16), (5.0, 3)):
            BO.check(BO.boundary(pts, nrm, r, g), *_boundary(t, r, nrm, g, what=(n, r)), what=(n, r))


def test_nan_cloud_and_every_point_deleted():
    n = 70
    nrm = _unit(np.random.default_rng(510), n)
    t = kdtree.New(np.full((n, 3), nan, f32))
    pts = synth.uniform_cloud(n, 1.0, 511)
    td = kdtree.New(pts)
    td.DeletePoints(np.arange(n))
    for tree in (t, td):
        ids, gaps, masks, counts = _boundary(tree, 0.5, nrm, 1)
        assert len(ids) == 0 and np.all(gaps == -1) and not masks.any() and not counts.any()
    BO.check(BO.boundary(pts, nrm, 0.5, 1, deleted=np.arange(n)), *_boundary(td, 0.5, nrm, 1))


def test_unusable_normals_among_good_ones():
    rng = np.random.default_rng(520)
    pts = synth.uniform_cloud(3000, 1.0, 521)
    nrm = _unit(rng, len(pts))
    bad = rng.permutation(len(pts))[:600].reshape(6, 100)
    nrm[bad[0]] = 0.0
    nrm[bad[1]] = -0.0
    nrm[bad[2], rng.integers(0, 3, 100)] = nan
    nrm[bad[3], rng.integers(0, 3, 100)] = inf
    nrm[bad[4], rng.integers(0, 3, 100)] = -inf
    nrm[bad[5]] *= f32(1e-30)  # tiny is not zero: evaluated
    t = kdtree.New(pts)
    ref = BO.boundary(pts, nrm, 0.12, 16)
    got = _boundary(t, 0.12, nrm, 16)
    BO.check(ref, *got)
    off = bad[:5].ravel()
    assert np.all(got[1][off] == -1) and not got[2][off].any() and not got[3][off].any() and not np.isin(got[0], off).any()
    assert np.all(got[1][bad[5]] >= 0) and len(got[0]) > 100


def test_min_neighbors_and_min_gap():
    pts = synth.uniform_cloud(2000, 1.0, 530)
    nrm = _unit(np.random.default_rng(531), len(pts))
    t = kdtree.New(pts)
    r = 0.15
    base = BO.boundary(pts, nrm, r, 16, 1)
    c = base["counts"]
    lo, mid, hi = int(c.min()), int(np.median(c)), int(c.max())
    assert lo < mid < hi
    for mn in (-3, 0, 1, lo, mid, hi, hi + 1):
        ref = BO.boundary(pts, nrm, r, 16, mn)
        got = _boundary(t, r, nrm, 16, mn, what=mn)
        BO.check(ref, *got, what=mn)
        assert np.array_equal(got[3], c)  # the count stays where only min_neighbors failed
        assert np.array_equal(got[1] == -1, c < max(mn, 1))
    assert len(_boundary(t, r, nrm, 16, hi + 1)[0]) == 0
    for g in (1, 64):
        BO.check(BO.boundary(pts, nrm, r, g), *_boundary(t, r, nrm, g, what=g), what=g)
    assert len(_boundary(t, r, nrm, 1)[0]) > len(_boundary(t, r, nrm, 16)[0]) > 0
    # min_gap 64 takes a point that sees nobody in any sector: one alone in its neighbourhood
    far = np.ascontiguousarray(np.concatenate([pts, f32([[5, 5, 5]])]))
    nf = np.concatenate([nrm, f32([[0, 0, 1]])])
    ids, gaps, masks, counts = _boundary(kdtree.New(far), r, nf, 64)
    assert ids.tolist() == [2000] and gaps[2000] == 64 and masks[2000] == 0 and counts[2000] == 1


def test_coincident_points():
    """ten points at one place (and one on the normal's line through them): no direction, mask 0, gap 64, flagged"""
    pts = np.ascontiguousarray(np.concatenate([np.tile(f32([0.5, 0.25, 0.125]), (10, 1)), f32([[0.5, 0.25, 0.375]])]))
    nrm = np.tile(f32([0, 0, 1]), (11, 1))
    t = kdtree.New(pts)
    for g in (1, 16, 64):
        ids, gaps, masks, counts = _boundary(t, 1.0, nrm, g)
        assert np.array_equal(ids, np.arange(11)) and np.all(gaps == 64) and not masks.any() and np.all(counts == 11)
        BO.check(BO.boundary(pts, nrm, 1.0, g), ids, gaps, masks, counts)


def test_bad_arguments():
    lib = L.lib()
    pts = synth.uniform_cloud(100, 1.0, 90)
    t = kdtree.New(pts)
    nrm = _unit(np.random.default_rng(91), 100)
    ids = np.zeros(100, np.int64)
    cnt = C.c_int64(5)

    def host(tree=t._h, r=0.2, nr=L.ptr(nrm), g=16, i=L.ptr(ids), c=C.byref(cnt)):
        return lib.pcgx_kdtree_boundary(tree, r, nr, g, 1, i, c, None, None, None)

    def dev(tree=t._h, r=0.2, nr=L.ptr(nrm), g=16, i=L.ptr(ids), c=L.ptr(ids)):  # (rejected before anything is read)
        return lib.pcgx_kdtree_boundary_dev(tree, r, nr, g, 1, i, c, None, None, None, None)
    for r in (0.0, -1.0, inf, nan):
        assert host(r=r) == L.PCGX_E_INVALID and dev(r=r) == L.PCGX_E_INVALID
    for g in (0, -1, 65, 1 << 20):
        assert host(g=g) == L.PCGX_E_INVALID and dev(g=g) == L.PCGX_E_INVALID
    for f in (host, dev):
        assert f(tree=None) == L.PCGX_E_INVALID
        assert f(nr=None) == L.PCGX_E_INVALID
        assert f(i=None) == L.PCGX_E_INVALID
        assert f(c=None) == L.PCGX_E_INVALID
    assert cnt.value == 5 and not ids.any()
    # the optional outputs may be left out: the same ids
    L.check(host())
    want = t.Boundary(0.2, nrm)[0]
    assert len(want) > 0 and np.array_equal(ids[:cnt.value], want) and np.all(ids[cnt.value:] == -1)
    with pytest.raises(ValueError):
        t.Boundary(0.2, nrm[:50])


# ------------------------------------------------------------------------------------------------ 6. loops

def test_loops_on_the_plate():
    pts, t, nrm, _ = _plate()
    be = features.BoundaryEstimation(t)
    be.SetRadiusSearch(BS.PLATE_RADIUS)
    be.SetInputNormals(nrm)
    be.SetAngleThreshold(np.pi / 2.0)
    be.SetMinNeighbors(1)
    ids = be.Compute()[0]
    assert np.array_equal(ids, t.Boundary(BS.PLATE_RADIUS, nrm, 16)[0])
    labels, sizes, members = be.Loops(2.0)
    print("loops:", sizes.tolist())
    assert len(sizes) == 3 and sizes[0] > sizes[1] >= sizes[2]  # the outer rim, then the holes
    assert np.array_equal(np.sort(members), ids) and int(sizes.sum()) == len(ids)  # every id once, and only boundary ids
    assert np.array_equal(np.nonzero(labels >= 0)[0], ids)
    d_outer = np.minimum(np.minimum(pts[:, 0], BS.PLATE_NX - 1 - pts[:, 0]), np.minimum(pts[:, 1], BS.PLATE_NY - 1 - pts[:, 1]))
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    groups = [members[cuts[k]:cuts[k + 1]] for k in range(3)]
    assert np.all(np.diff(groups[0]) > 0) and all(np.all(labels[g] == k) for k, g in enumerate(groups))
    assert np.all(d_outer[groups[0]] < 1.5)  # the largest group is the outer rim
    for g, (c, rad) in zip(groups[1:], BS.PLATE_HOLES):  # the larger hole before the smaller
        assert np.all(np.abs(np.hypot(pts[g, 0] - c[0], pts[g, 1] - c[1]) - rad) < 1.5)
    assert len(be.Loops(2.0, MinSize=int(sizes[1]) + 1)[1]) == 1
