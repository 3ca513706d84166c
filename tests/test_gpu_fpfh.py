"""FPFH descriptors on the GPU (pcgx_kdtree_fpfh / _dev, csrc/fpfh.hip) against the float64 oracle
(tests/fpfh_oracle.py): the SPFH counts within the oracle's admissible bounds -- equalities on these scenes, which have
no fragile pair (tests/test_fpfh_oracle.py) --, the pair counts, and the descriptors within 2^-22 relative with zeros
exact, on every kind of handle, at fat grid rows, with counters past 65 535, and under an exact rigid motion."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import kdtree, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_oracle as FO  # noqa: E402
import normals_oracle as NO  # noqa: E402
from test_fpfh_oracle import scenes  # noqa: E402
from test_gpu_radius_edges import BOX, HC, _assert_heap_grid, _grid_on  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64

_CACHE = {}


def _cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _scene(name):
    return _cached("scene", scenes)[name]


def _oracle_all(P, N, r, deleted=None):
    """the oracle's rows for every point of the cloud, brute-force lists (a deleted point is nobody's neighbour)"""
    pts = np.array(P, f32)
    if deleted is not None:
        pts[deleted] = np.nan
    offs, ids = NO.brute_force_lists(pts, P, r)
    return FO.fpfh(P, N, np.arange(len(P)), offs, ids)


def _range_counts(t, q, radius):
    q = L.f32c(q).reshape(-1, 3)
    c = np.zeros(len(q), np.int64)
    L.check(L.lib().pcgx_kdtree_range_count(t._h, L.ptr(q), len(q), float(radius), L.ptr(c)))
    return c


def test_surface_on_every_kind_of_handle(monkeypatch):
    P, N, r = _scene("surface")
    assert len(P) % 64 == 56  # a partial last wave
    ref = _cached("surface ref", lambda: _oracle_all(P, N, r))
    assert 25 < ref["n_valid"] / len(P) < 40
    t = kdtree.New(P)
    FO.check(ref, *t.FPFH(r, N), what="surface grid")
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    FO.check(ref, *t.FPFH(r, N), what="surface walk")
    monkeypatch.delenv("PCGX_RANGE_WALK")
    gone = np.random.default_rng(5).choice(len(P), len(P) // 10, replace=False)
    td = kdtree.New(P)
    td.DeletePoints(gone)
    refd = _oracle_all(P, N, r, gone)
    assert refd["n_fragile"] == 0
    f, c, m = td.FPFH(r, N)
    FO.check(refd, f, c, m, what="surface deleted")
    # N(q) is the set range_count counts on that handle: with unit normals on a surface every neighbour but the point
    # itself is a valid pair (a deleted query does not find itself)
    own = np.ones(len(P), np.int64)
    own[gone] = 0
    assert np.array_equal(m, _range_counts(td, P, r) - own)
    assert not np.array_equal(refd["counts"], ref["counts"])


def test_sphere_every_pair_a_swap_tie():
    P, N, r = _scene("sphere")
    FO.check(_oracle_all(P, N, r), *kdtree.New(P).FPFH(r, N), what="sphere")


@pytest.mark.parametrize("name", ["cube", "lattice"])
def test_cube_and_lattice(name):
    P, N, r = _scene(name)
    ref = _oracle_all(P, N, r)
    f, c, m = kdtree.New(P).FPFH(r, N)
    FO.check(ref, f, c, m, what=name)
    if name == "lattice":  # every pair exactly mid-bin: 100 + 100 in bin 5 of every feature
        assert np.all(c[:, :, 5] == m[:, None]) and m.min() > 0
        assert np.array_equal(f.reshape(-1, 3, 11)[:, :, 5], np.full((len(P), 3), 200.0, f32))


def test_normals_from_the_library_and_device_entry_point():
    import torch
    P0, _, r = _scene("surface")
    far = (np.arange(20, dtype=f32)[:, None] * f32(2.0) + f32(10.0)) * np.ones((1, 3), f32)  # 20 isolated points
    P = np.ascontiguousarray(np.concatenate([P0, far]), f32)
    t = kdtree.New(P)
    vp = (0.8, 0.8, 50.0)
    N = t.Normals(r, Viewpoint=vp)[0]
    zero = np.all(N == 0, axis=1)
    assert zero[-20:].all() and zero.sum() >= 20
    f, c, m = t.FPFH(r, N)
    FO.check(_oracle_all(P, N, r), f, c, m, what="estimated normals")
    assert np.all(m[zero] == 0) and np.all(f[zero] == 0) and np.all(c[zero] == 0)
    assert m[~zero].min() > 0
    # NormalsDev -> FPFHDev on one stream, nothing copied to the host in between: the host entry point's bits
    dev = torch.device("cuda", 0)
    dn = torch.empty((len(P), 3), dtype=torch.float32, device=dev)
    df = torch.empty((len(P), 33), dtype=torch.float32, device=dev)
    dc = torch.empty((len(P), 33), dtype=torch.int32, device=dev)
    dm = torch.empty(len(P), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    t.NormalsDev(r, dn.data_ptr(), Viewpoint=vp, stream=st)
    t.FPFHDev(r, dn.data_ptr(), df.data_ptr(), dc.data_ptr(), dm.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(dn.cpu().numpy().view(np.uint32), N.view(np.uint32))
    assert np.array_equal(df.cpu().numpy().view(np.uint32), f.view(np.uint32))
    assert np.array_equal(dc.cpu().numpy().reshape(-1, 3, 11), c) and np.array_equal(dm.cpu().numpy(), m)
    # without the optional outputs
    df2 = torch.zeros((len(P), 33), dtype=torch.float32, device=dev)
    t.FPFHDev(r, dn.data_ptr(), df2.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(df2.cpu().numpy().view(np.uint32), f.view(np.uint32))


def test_zero_and_nan_normals_among_live_points(monkeypatch):
    """Points WITH neighbours whose normals are zero, NaN or infinite (how degenerate points come out of Normals, and
    worse): every pair they are part of is invalid, so their own rows have m == 0 and no counts, yet F is the
    neighbours' term alone (0 + 100 W / T: 100 per feature); their neighbours lose those pairs, and take nothing
    from them in W (a record with m_i == 0 must be skipped, not divided by).  On every kind of handle."""
    P, N0, r = _scene("surface")
    N = N0.copy()
    bad = np.random.default_rng(12).choice(len(P), 60, replace=False)
    N[bad[:30]] = 0
    N[bad[30:45], 1] = np.nan
    N[bad[45:], 0] = np.inf
    ref = _oracle_all(P, N, r)
    clean = _cached("surface ref", lambda: _oracle_all(P, N0, r))
    assert ref["n_fragile"] == 0
    assert np.all(ref["pairs"][bad] == 0) and np.all(clean["pairs"][bad] >= 6)
    touched = ref["pairs"] < clean["pairs"]
    touched[bad] = False
    assert touched.sum() >= 500  # live points with such a neighbour
    gone = np.setdiff1d(np.random.default_rng(5).choice(len(P), len(P) // 10, replace=False), bad)
    t = kdtree.New(P)
    td = kdtree.New(P)
    td.DeletePoints(gone)
    for name, h, want in (("grid", t, ref), ("walk", t, ref), ("deleted", td, _oracle_all(P, N, r, gone))):
        if name == "walk":
            monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        f, c, m = h.FPFH(r, N)
        monkeypatch.delenv("PCGX_RANGE_WALK", raising=False)
        FO.check(want, f, c, m, what="zero / NaN normals, " + name)
        assert np.all(m[bad] == 0) and np.all(c[bad] == 0)
        assert np.all(m[touched] > 0) and np.all(np.isfinite(f))
        # the rows of the bad points: the neighbour term alone, 100 per feature
        sums = f[bad].astype(f64).reshape(-1, 3, 11).sum(axis=2)
        assert np.all(np.abs(sums - 100.0) <= 1e-4), name
        assert np.all(np.abs(f[bad].astype(f64) - want["fpfh"][bad]) <= FO.FLOAT_TOL * want["fpfh"][bad]), name
        # a live point's row: both terms
        sums = f[touched].astype(f64).reshape(-1, 3, 11).sum(axis=2)
        assert np.all(np.abs(sums - 200.0) <= 2e-4), name


# ------------------------------------------------------------------------------------------------ fat rows

# Four heaps of coincident records round HC, each alone in its grid row (the layout of
# tests/test_gpu_radius_edges.py::_heap_scene: they differ by 1.0 in y or z, more than R_HEAP apart): 4095 records are
# one lane's row, 4096 and 4097 a fat row the wave shares; their records carry random unit normals.  The 70 000 records
# of the fourth share one normal: a background point beside it has 70 000 pairs in one bin of every feature, which a
# 16-bit counter would wrap.
R_HEAP = 1.0
HEAP_AT = [HC + np.array(o, f32) for o in ((0.0, -0.5, -0.5), (0.25, 0.5, -0.5), (-0.25, -0.5, 0.5), (0.5, 0.5, 0.5))]
HEAP_SIZE = [4095, 4096, 4097, 70_000]


def _heap_scene():
    """-> points, normals (shuffled), and the oracle's view of them: sites (every background point and every record of
    the three small heaps on its own, the big heap once), mult (how many records a site stands for), first (a point id
    of each site), big (the ids of the big heap's records)."""
    rng = np.random.default_rng(2025)
    slab = synth.uniform_cloud(5600, 1.0, 31) * np.array([BOX, BOX, 4.0], f32)  # background, z in [0, 4): sparse
    s = (rng.uniform(6.5, 9.5, (3000, 3)) + np.array([0.0, 0.0, 4.0])).astype(f32)  # round the heaps ...
    clear = np.ones(len(s), bool)
    for h in HEAP_AT:  # ... but never in a heap's row
        clear &= (np.abs(s[:, 1] - h[1]) >= 0.5) | (np.abs(s[:, 2] - h[2]) >= 0.5)
    bg = np.concatenate([slab, s[clear][:400], np.array([[0.0, 0.0, 0.0], [BOX, BOX, BOX]], f32)]).astype(f32)
    parts = [bg] + [np.repeat(h[None, :], m, axis=0) for h, m in zip(HEAP_AT, HEAP_SIZE)]
    pts = np.concatenate(parts).astype(f32)
    nrm = rng.standard_normal((len(pts), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm.astype(f32)
    n_big0 = len(pts) - HEAP_SIZE[3]
    nrm[n_big0:] = nrm[n_big0]
    perm = rng.permutation(len(pts))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(pts))  # unshuffled index -> point id
    sites = np.arange(n_big0 + 1)  # unshuffled indices of the sites
    mult = np.ones(len(sites), np.int64)
    mult[-1] = HEAP_SIZE[3]
    return dict(points=np.ascontiguousarray(pts[perm]), normals=np.ascontiguousarray(nrm[perm]), n_bg=len(bg),
                first=inv[sites], mult=mult, big=inv[n_big0:])


def _heap_reference():
    """the oracle over the sites: a background site's list is every other site within R_HEAP; a heap record's list is
    its heap's site list (its heap-mates are at DistSq == 0: invalid pairs, and no weight in the FPFH)"""
    sc = _cached("heaps", _heap_scene)
    P, N = sc["points"][sc["first"]], sc["normals"][sc["first"]]
    ns, n_bg = len(P), sc["n_bg"]
    bound = f32(R_HEAP) * f32(R_HEAP)
    lists = []
    for k in range(n_bg):
        d = NO.dist_sq_f32(P, P[k])
        lists.append(np.nonzero((d < bound) & (d > 0))[0])
    at = n_bg
    for h, m in zip(HEAP_AT, HEAP_SIZE[:3] + [1]):
        d = NO.dist_sq_f32(P, h)
        lists += [np.nonzero((d < bound) & (d > 0))[0]] * m
        at += m
    assert at == ns
    offs = np.zeros(ns + 1, np.int64)
    np.cumsum([len(a) for a in lists], out=offs[1:])
    ids = np.concatenate(lists).astype(np.int64)
    res = FO.fpfh(P, N, np.arange(ns), offs, ids, mult=sc["mult"][ids])
    res["near_heap"] = np.array([np.any(a >= n_bg) for a in lists[:n_bg]])
    res["two_heaps"] = np.array([len(np.unique(np.searchsorted(np.cumsum([n_bg] + HEAP_SIZE[:3]), a[a >= n_bg], side="right"))) >= 2
                                 for a in lists[:n_bg]])
    return res


@pytest.mark.parametrize("grid", [None, "2"])
def test_fat_rows_and_wide_counters(grid, monkeypatch):
    """Every background point (about 6000: some 120 within R_HEAP of a heap, some of them of two) and every record of
    the heaps.  grid None: the library's own choice for this cloud, which is the tree walk -- the heaps crowd the grid
    and the handle drops it (asserted).  PCGX_GRID=2 keeps the grid: this is the grid path, rows of 4095 records scanned
    by one lane, 4096, 4097 and 70 000 by the wave (asserted: the grid is on, every heap has a row of its own)."""
    sc = _cached("heaps", _heap_scene)
    ref = _cached("heaps ref", _heap_reference)
    n_bg = sc["n_bg"]
    assert ref["near_heap"].sum() >= 100 and ref["two_heaps"].sum() >= 5 and (~ref["near_heap"]).sum() >= 1000
    assert ref["counts"][:n_bg].max() > 65_535 + 4097  # one bin past 16 bits from the big heap alone
    if grid:
        monkeypatch.setenv("PCGX_GRID", grid)
    t = kdtree.New(sc["points"])
    if grid:
        _assert_heap_grid(t)
    else:
        assert _grid_on(t)[3] == 0  # no grid: the walk
    assert ref["n_fragile"] == 0
    f, c, m = t.FPFH(R_HEAP, sc["normals"])
    FO.check(ref, f[sc["first"]], c[sc["first"]], m[sc["first"]], what="heaps, PCGX_GRID=%s" % grid)
    # the 70 000 records of the big heap are one point with one normal: one row, 70 000 times
    big = sc["big"]
    assert np.all(f[big].view(np.uint32) == f[big[0]].view(np.uint32)) and np.all(c[big] == c[big[0]]) and np.all(m[big] == m[big[0]])
    # a heap's records do not pair with their heap-mates
    assert m[sc["first"]][n_bg:].max() < 200


def test_exact_rigid_motion():
    """A cloud on the 2^-10 lattice, turned by 90 degrees about z and shifted by multiples of 1/4, normals turned with
    it: every difference, DistSq ((dx^2 + dy^2) + dz^2 commutes in x and y) and neighbour set is the same, so the
    counts are equal exactly and the descriptors within the contract's bound of each other."""
    rng = np.random.default_rng(77)
    xy = rng.integers(0, 1690, (3000, 2)).astype(f64) / 1024.0
    x, y = xy[:, 0], xy[:, 1]
    z = np.rint((0.5 * np.sin(0.7 * x) * np.cos(0.5 * y) + 0.3 * np.sin(1.3 * y)) * 1024.0) / 1024.0
    P = np.ascontiguousarray(np.stack([x, y, z], axis=1), f32)
    _, N = synth.surface_cloud(3000, 1.65, 8)
    P2 = np.ascontiguousarray(np.stack([-P[:, 1], P[:, 0], P[:, 2]], axis=1) + np.array([2.25, -0.5, 1.75], f32), f32)
    N2 = np.ascontiguousarray(np.stack([-N[:, 1], N[:, 0], N[:, 2]], axis=1), f32)
    assert np.array_equal(P2.astype(f64) - np.array([2.25, -0.5, 1.75]), np.stack([-P[:, 1], P[:, 0], P[:, 2]], axis=1).astype(f64))
    r = 0.1
    ref, ref2 = _oracle_all(P, N, r), _oracle_all(P2, N2, r)
    assert ref["n_fragile"] == 0 and ref2["n_fragile"] == 0 and ref["n_valid"] > 50_000
    f, c, m = kdtree.New(P).FPFH(r, N)
    f2, c2, m2 = kdtree.New(P2).FPFH(r, N2)
    FO.check(ref, f, c, m, what="lattice cloud")
    FO.check(ref2, f2, c2, m2, what="lattice cloud, moved")
    assert np.array_equal(c, c2) and np.array_equal(m, m2)
    a, b = f.astype(f64), f2.astype(f64)
    assert np.all(np.abs(a - b) <= FO.FLOAT_TOL * a)


def test_bad_arguments_and_determinism():
    P, N, r = _scene("cube")
    t = kdtree.New(P)
    lib = L.lib()
    n = len(P)
    out = np.empty((n, 33), f32)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.pcgx_kdtree_fpfh(t._h, L.ptr(N), bad, L.ptr(out), None, None) == L.PCGX_E_INVALID
        assert lib.pcgx_kdtree_fpfh_dev(t._h, C.c_void_p(16), bad, C.c_void_p(16), None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fpfh(t._h, None, r, L.ptr(out), None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fpfh(t._h, L.ptr(N), r, None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fpfh_dev(t._h, None, r, C.c_void_p(16), None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fpfh_dev(t._h, C.c_void_p(16), r, None, None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fpfh(None, L.ptr(N), r, L.ptr(out), None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fpfh_dev(None, C.c_void_p(16), r, C.c_void_p(16), None, None, None) == L.PCGX_E_INVALID
    with pytest.raises(ValueError):
        t.FPFH(r, N[:-1])
    # the optional outputs may be left out; two runs give the same bits
    assert lib.pcgx_kdtree_fpfh(t._h, L.ptr(N), r, L.ptr(out), None, None) == L.PCGX_OK
    f, c, m = t.FPFH(r, N)
    f2, c2, m2 = t.FPFH(r, N)
    assert np.array_equal(out.view(np.uint32), f.view(np.uint32))
    assert np.array_equal(f.view(np.uint32), f2.view(np.uint32)) and np.array_equal(c, c2) and np.array_equal(m, m2)
    # (Len() == 0 is PCGX_OK by the contract, but no handle can be empty: pcgx_kdtree_build refuses one,
    # tests/test_gpu_kdtree.py)  A tree of one point: Len() == 1, an isolated point, 33 zeros
    f1, c1, m1 = kdtree.New(P[:1]).FPFH(r, N[:1])
    assert np.all(f1 == 0) and np.all(c1 == 0) and m1[0] == 0
