"""Ray queries on the GPU (KDTree.RayCast / RayPierce and their device forms, pcgol_amd/rays.py) against the NumPy oracle
(tests/rays_oracle.py): ids, along, off_sq and counts by array_equal -- a minimum under a total order and an integer sum
over a set have no tolerance --, on the grid, the forced walk and after DeletePoints, and the same bits from a second
call."""
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import kdtree, rays, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays_oracle as RO  # noqa: E402
import rays_scenes as RS  # noqa: E402
from test_gpu_radius_edges import HEAPS, _grid_on, _handles, _heap_deleted, _heap_scene  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
nan, inf = np.nan, np.inf


def _cast(t, o, d, rho, s_min=None, s_max=None, what=""):
    """RayCast, and the same bits from a second call"""
    got = t.RayCast(o, d, rho, s_min, s_max)
    again = t.RayCast(o, d, rho, s_min, s_max)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), what
    return got


def _pierce(t, o, d, rho, s_min=None, s_max=None, what=""):
    got = t.RayPierce(o, d, rho, s_min, s_max)
    assert np.array_equal(got, t.RayPierce(o, d, rho, s_min, s_max)), what
    return got


def _check(t, pts, o, d, rho, s_min=None, s_max=None, deleted=None, what="", ref=None):
    """both modes against the oracle (ref: its answer where a test has it already) -> (ids, along, off_sq, counts)"""
    hits, wc = ref if ref is not None else RO.query(pts, o, d, rho, s_min, s_max, deleted)
    got = _cast(t, o, d, rho, s_min, s_max, what)
    for g, w, name in zip(got, hits[0], ("ids", "along", "off_sq")):
        assert np.array_equal(g, w), (what, name, np.nonzero(g != w)[0][:8])
    counts = _pierce(t, o, d, rho, s_min, s_max, what)
    assert np.array_equal(counts, wc), (what, "counts", np.nonzero(counts != wc)[0][:8])
    return got + (counts,)


def _with_filler(pts, seed, lo=(50.0, 50.0, 50.0), n=3000):
    """pts, then a uniform cloud far from them: enough points for a grid, ids of pts unchanged"""
    return np.ascontiguousarray(np.concatenate([np.asarray(pts, f32), synth.uniform_cloud(n, 4.0, seed) + f32(lo)]), f32)


def _geometry(t):
    geom, dims = np.zeros(5, f32), np.zeros(3, np.int32)
    L.check(L.lib().pcgx_debug_grid_geometry(t._h, L.ptr(geom), L.ptr(dims)))
    return geom, dims


# ------------------------------------------------------------------------------------------------ 1. the lattice

def test_lattice(monkeypatch):
    pts = RS.lattice()
    o, d, s_min, s_max, ids, along, off, counts = RS.lattice_rays()
    for what, t, _ in _handles(pts, monkeypatch, rows=False):
        got = _check(t, pts, o, d, RS.LATTICE_RHO, s_min, s_max, what=what)
        assert np.array_equal(got[0], ids) and np.array_equal(got[1], along) and np.array_equal(got[2], off), what
        assert np.array_equal(got[3], counts), what
    gone = np.unique(ids[ids >= 0])
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    got = _check(td, pts, o, d, RS.LATTICE_RHO, s_min, s_max, deleted=gone, what="deleted")
    assert got[0][0] == RS.lattice_id(1, 0, 0) and got[1][0] == 2.0 and got[0][9] == RS.lattice_id(0, 1, 6)


# ------------------------------------------------------------------------------------------------ 2. a surface scene

def _surface_rays(n_rays=2000, seed=8):
    rng = np.random.default_rng(seed)
    vp = f32([2.5, 2.5, 9.0])  # above the surface z = h(x, y), |h| < 0.8, over [0, 5)^2
    aim = np.concatenate([rng.uniform(-1.0, 6.0, (n_rays, 2)), rng.uniform(-0.5, 0.5, (n_rays, 1))], axis=1).astype(f32)
    o = np.ascontiguousarray(np.broadcast_to(vp, aim.shape))
    return o, np.ascontiguousarray(aim - vp)


def test_surface_scene_on_every_handle(monkeypatch):
    pts = synth.surface_cloud(20_000, 5.0, 33)[0]
    o, d = _surface_rays()
    rho = 0.04  # about the points' spacing, 5 / sqrt(20 000)
    t = kdtree.New(pts)
    assert _grid_on(t)[3] == 1
    ref = RO.query(pts, o, d, rho, ranks=2)  # (one brute force for the grid, the walk and the second members)
    ids, along, off, counts = _check(t, pts, o, d, rho, what="grid", ref=ref)
    hit = ids >= 0
    assert 0.3 < hit.mean() < 0.9 and counts.max() >= 2  # rays outside the square miss; tubes hold several points
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    _check(t, pts, o, d, rho, what="walk", ref=ref)
    monkeypatch.delenv("PCGX_RANGE_WALK")
    # every first hit deleted: the new first hits are the oracle's second members, deleted ids count 0
    gone = np.unique(ids[hit])
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    after = _check(td, pts, o, d, rho, deleted=gone, what="deleted")
    second = ref[0][1]
    same = ~np.isin(second[0], gone)  # (a ray whose second member was another ray's first hit moves on further)
    assert same.mean() > 0.8 and all(np.array_equal(a[same], b[same]) for a, b in zip(after[:3], second))
    assert not after[3][gone].any() and not np.isin(after[0], gone).any()
    assert not np.array_equal(after[0], ids)


# ------------------------------------------------------------------------------------------------ 3. ties

def test_ties_go_to_the_smallest_id(monkeypatch):
    """coincident points with different ids, and mirror pairs at equal a, in both id orders"""
    special = f32([[1, 0, 0], [1, 0, 0], [1, 0, 0],          # 0..2 coincident on ray 0
                   [3, 0.25, 0], [3, -0.25, 0],              # 3, 4 a mirror pair on ray 0, behind
                   [0, 5, 0.25], [0, 5, -0.25], [0, 5, 0.25],  # 5..7 on ray 1: a pair and a copy
                   [2, 9, 2], [2, 9, 2]])                    # 8, 9 coincident on ray 2
    pts = _with_filler(special, 71)
    o = f32([[-1, 0, 0], [0, 3, 0], [2, 12, 2], [4, 0, 0]])
    d = f32([[1, 0, 0], [0, 2, 0], [0, -1, 0], [-1, 0, 0]])  # ray 3 meets the mirror pair first
    gone = np.array([0, 3, 5, 8])
    for what, t, dl in _handles(pts, monkeypatch, deleted=gone, rows=False):
        ids = _check(t, pts, o, d, 0.5, deleted=dl, what=what)[0]
        assert list(ids) == ([0, 5, 8, 3] if dl is None else [1, 6, 9, 4]), what
    small = kdtree.New(special)  # fewer than 64 points: no grid
    assert list(_check(small, special, o, d, 0.5, what="small")[0]) == [0, 5, 8, 3]


# ------------------------------------------------------------------------------------------------ 4. collinear points

@pytest.mark.parametrize("spacing", ["rho", "2rho", "h", "0.37rho"])
def test_collinear_points_on_slab_borders(spacing, monkeypatch):
    """A thousand points on the ray itself, evenly spaced: whatever the slab length, many fall on or beside slab borders.
    Each is counted exactly once, and the first hit is the first at or after s_min."""
    rho = 2.0 ** -5
    back = synth.uniform_cloud(3000, 1.0, 17) * f32([40, 4, 4]) + f32([0, 1, 1])  # away from the line y = z = 0
    sp = {"rho": rho, "2rho": 2 * rho, "0.37rho": 0.37 * rho}.get(spacing)
    if sp is None:  # the cell edge of the grid such a scene gets
        monkeypatch.setenv("PCGX_GRID", "2")
        line = np.zeros((1000, 3), f32)
        line[:, 0] = np.arange(1000) * f32(2 * rho)
        sp = float(_geometry(kdtree.New(np.concatenate([line, back])))[0][3])
    line = np.zeros((1000, 3), f32)
    line[:, 0] = (np.arange(1000) * sp).astype(f32)
    pts = np.ascontiguousarray(np.concatenate([line, back]))
    x = line[:, 0].astype(f64)
    o = f32([[-1, 0, 0], [x[-1] + 2, 0, 0], [-1, 0, 0]])
    d = f32([[1, 0, 0], [-0.5, 0, 0], [3, 0, 0]])
    s_min = f32([0, 0, (1 + 10.5 * sp) / 3])
    for what, t, _ in _handles(pts, monkeypatch, rows=False):
        ids, along, off, counts = _check(t, pts, o, d, rho, s_min, None, what=what)
        assert list(ids[:2]) == [0, 999] and ids[2] == 11 and not off.any(), what
        assert np.array_equal(counts[:1000], np.where(np.arange(1000) >= 11, 3, 2)), what
        assert not counts[1000:].any(), what


# ------------------------------------------------------------------------------------------------ 5. surface and ends

def test_tube_surface_and_range_ends(monkeypatch):
    p, s_min, s_max, member = RS.dyadic()
    n = len(p)
    o = np.zeros((n, 3), f32)
    d = np.tile(f32(RS.DYADIC_D), (n, 1))
    trees = [("small", kdtree.New(p), p)]
    big = _with_filler(p, 72)
    trees += [(what, t, big) for what, t, _ in _handles(big, monkeypatch, rows=False)]
    for what, t, pts in trees:
        if what == "walk":
            monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        _check(t, pts, o, d, RS.DYADIC_RHO, s_min, s_max, what=what)
        for i in range(n):  # row i: its own point under its own range
            c = t.RayPierce(o[i:i + 1], d[i:i + 1], RS.DYADIC_RHO, s_min[i:i + 1], s_max[i:i + 1])
            assert bool(c[i]) == bool(member[i]), (what, i)
        monkeypatch.delenv("PCGX_RANGE_WALK", raising=False)


# ------------------------------------------------------------------------------------------------ 6. far off, hair-thin

def test_far_off_cloud(monkeypatch):
    """+4096 on every axis, rho = 2^-6: the float32 centre of a ball is 2^-12 coarse there, the cover's margin grows"""
    pts = synth.surface_cloud(20_000, 5.0, 35)[0] * f32(0.5) + f32(4096)
    o, d = _surface_rays(600, 9)
    o, d = o * f32(0.5) + f32(4096), d * f32(0.5)
    ref = RO.query(pts, o, d, 2.0 ** -6)
    for what, t, _ in _handles(pts, monkeypatch, rows=False):
        ids = _check(t, pts, o, d, 2.0 ** -6, what=what, ref=ref)[0]
        assert (ids >= 0).mean() > 0.3, what


def test_hair_thin_ray_across_a_long_cloud(monkeypatch):
    """rho = 1e-4 across 100 units: 500 000 slabs of 2 rho -- the cap of 4096 lengthens them on the walks (on the grid a
    slab is a cell long and there are fewer); the ray is answered exactly either way"""
    rng = np.random.default_rng(12)
    cloud = synth.uniform_cloud(20_000, 1.0, 19) * f32([100, 1, 1])
    on = np.stack([rng.uniform(0, 100, 1500), np.full(1500, 0.5), np.full(1500, 0.5)], axis=1).astype(f32)
    near = on[:500] + f32([0, 1.5e-4, 0])  # just outside the hair
    pts = np.ascontiguousarray(np.concatenate([cloud, on, near]))
    o = f32([[-1, 0.5, 0.5], [101, 0.5, 0.5], [-1, 0.4, 0.45]])
    d = f32([[102, 0, 0], [-51, 0, 0], [102, 0.2, 0.2]])  # the last one crosses the cloud at a slant, 0.05 from the line
    gone = np.arange(20_000, 20_200)
    for what, t, dl in _handles(pts, monkeypatch, deleted=gone, rows=False):
        counts = _check(t, pts, o, d, 1e-4, 0.0, f32(2.0), deleted=dl, what=what)[3]
        assert counts[20_000:21_500].sum() == 2 * (1500 - (0 if dl is None else 200)) and not counts[21_500:].any(), what


# ------------------------------------------------------------------------------------------------ 7. the contract's edges

def _edge_rays():
    o = np.tile(f32([-1, 0.5, 0.5]), (16, 1))
    d = np.tile(f32([1, 0.01, 0.02]), (16, 1))
    s_min, s_max = np.zeros(16, f32), np.full(16, inf, f32)
    o[1] = [5, 5, 5]             # misses the box
    o[2] = [0.5, 0.5, 0.5]       # starts inside it
    d[3] = [-1, 0, 0]            # points away
    d[4] = [-1, 0, 0]            # ... and a negative s_min brings it back
    s_min[4], s_max[4] = -3, -1.2
    d[5] = 0                     # dd == 0
    d[6, 1] = nan
    d[7, 0] = inf
    o[8, 2] = nan
    o[9, 0] = -inf
    s_min[10], s_max[10] = 2, 1  # s_min > s_max
    s_min[11] = nan
    s_max[12] = nan
    s_min[13], s_max[13] = -inf, inf
    s_min[14] = s_max[14] = 1.5  # a range of one point
    d[15] = [1e-20, 1e-22, 2e-22]  # a tiny direction
    return o, d, s_min, s_max


def test_contract_edges(monkeypatch):
    o, d, s_min, s_max = _edge_rays()
    pts = synth.uniform_cloud(4000, 1.0, 41)
    for what, t, dl in _handles(pts, monkeypatch, deleted=np.arange(0, 4000, 7), rows=False):
        ids = _check(t, pts, o, d, 0.05, s_min, s_max, deleted=dl, what=what)[0]
        assert ids[0] >= 0 and ids[2] >= 0 and ids[4] >= 0 and ids[13] >= 0 and ids[15] >= 0, what
        assert np.all(ids[[1, 3, 5, 6, 7, 8, 9, 10, 11, 12]] == -1), what
        got = t.RayCast(o, d, 0.05)  # s_min and s_max left out: 0 and +inf
        assert all(np.array_equal(a, b) for a, b in zip(got, RO.raycast(pts, o, d, 0.05, deleted=dl))), what
    # fewer than 64 points (no grid), NaN and infinite points among finite ones
    for n in (1, 2, 63):
        small = pts[:n].copy()
        _check(kdtree.New(small), small, o, d, 0.3, s_min, s_max, what=n)
    bad = pts[:500].copy()
    bad[::9, 1] = nan
    bad[4::9, 0] = inf
    bad[0] = nan  # (the first point too: the build's own box starts there)
    tb = kdtree.New(bad)
    got = _check(tb, bad, o, d, 0.1, s_min, s_max, what="nan points")
    assert (got[0] >= 0).sum() >= 3 and not got[3][::9].any()
    infs = pts[:500].copy()  # infinite points only
    infs[4::9, 0] = inf
    infs[7::9, 2] = -inf
    ti = kdtree.New(infs)
    got = _check(ti, infs, o, d, 0.1, s_min, s_max, what="inf points")
    assert (got[0] >= 0).sum() >= 3 and not got[3][4::9].any()
    ti.DeletePoints(np.arange(0, 500, 5))
    _check(ti, infs, o, d, 0.1, s_min, s_max, deleted=np.arange(0, 500, 5), what="inf points, deleted")
    tb.DeletePoints(np.arange(1, 500, 5))
    _check(tb, bad, o, d, 0.1, s_min, s_max, deleted=np.arange(1, 500, 5), what="nan points, deleted")
    allnan = np.full((70, 3), nan, f32)
    got = _check(kdtree.New(allnan), allnan, o, d, 0.1, what="all nan")
    assert np.all(got[0] == -1) and not got[3].any()
    # every point deleted
    td = kdtree.New(pts[:200].copy())
    td.DeletePoints(np.arange(200))
    got = _check(td, pts[:200], o, d, 0.3, deleted=np.arange(200), what="all deleted")
    assert np.all(got[0] == -1) and not got[1].any() and not got[3].any()
    with pytest.raises(L.ErrNoPoint):  # Len() == 0 cannot be built: the reference panics there
        kdtree.New(np.zeros((0, 3), f32))
    # nr == 0
    t = kdtree.New(pts)
    got = t.RayCast(np.zeros((0, 3), f32), np.zeros((0, 3), f32), 0.1)
    assert all(len(g) == 0 for g in got)
    assert not t.RayPierce(np.zeros((0, 3), f32), np.zeros((0, 3), f32), 0.1).any()


def test_optional_outputs_and_bad_arguments():
    lib = L.lib()
    pts = synth.uniform_cloud(100, 1.0, 90)
    t = kdtree.New(pts)
    o, d = np.tile(f32([-1, 0.5, 0.5]), (5, 1)), np.tile(f32([1, 0, 0]), (5, 1))
    d[:, 1] = np.linspace(-0.2, 0.2, 5)
    want = RO.raycast(pts, o, d, 0.2)
    assert (want[0] >= 0).any()
    ids, along, off = np.full(5, -7, np.int64), np.full(5, -7.0), np.full(5, -7.0)
    counts = np.zeros(100, np.int32)

    def cast(tree=t._h, po=L.ptr(o), pd=L.ptr(d), nr=5, r=0.2, i=L.ptr(ids), a=L.ptr(along), f=L.ptr(off)):
        return lib.pcgx_kdtree_raycast(tree, po, pd, None, None, nr, r, i, a, f)

    def cast_dev(tree=t._h, po=L.ptr(o), pd=L.ptr(d), nr=5, r=0.2, i=L.ptr(ids)):  # (rejected before anything is read)
        return lib.pcgx_kdtree_raycast_dev(tree, po, pd, None, None, nr, r, i, None, None, None)

    def pierce(tree=t._h, po=L.ptr(o), pd=L.ptr(d), nr=5, r=0.2, c=L.ptr(counts)):
        return lib.pcgx_kdtree_ray_pierce(tree, po, pd, None, None, nr, r, c)

    def pierce_dev(tree=t._h, po=L.ptr(o), pd=L.ptr(d), nr=5, r=0.2, c=L.ptr(counts)):
        return lib.pcgx_kdtree_ray_pierce_dev(tree, po, pd, None, None, nr, r, c, None)
    for f in (cast, cast_dev, pierce, pierce_dev):
        for r in (0.0, -1.0, inf, nan):
            assert f(r=r) == L.PCGX_E_INVALID
        assert f(tree=None) == L.PCGX_E_INVALID
        assert f(po=None) == L.PCGX_E_INVALID
        assert f(pd=None) == L.PCGX_E_INVALID
        assert f(nr=-1) == L.PCGX_E_INVALID
    assert cast(i=None) == L.PCGX_E_INVALID and cast_dev(i=None) == L.PCGX_E_INVALID
    assert pierce(c=None) == L.PCGX_E_INVALID and pierce_dev(c=None) == L.PCGX_E_INVALID
    assert np.all(ids == -7) and not counts.any()
    for f in (cast, cast_dev, pierce, pierce_dev):  # nr == 0 is fine, with nothing to point at
        assert f(po=None, pd=None, nr=0) == L.PCGX_OK
    # each optional output left out: the same ids, and the other output
    for a, f in ((None, None), (L.ptr(along), None), (None, L.ptr(off))):
        ids[:], along[:], off[:] = -7, -7.0, -7.0
        L.check(cast(a=a, f=f))
        assert np.array_equal(ids, want[0])
        assert np.array_equal(along, want[1]) if a else np.all(along == -7.0)
        assert np.array_equal(off, want[2]) if f else np.all(off == -7.0)
    with pytest.raises(ValueError):
        t.RayCast(o, d[:3], 0.2)


def test_more_rays_than_16_bits():
    """70 000 rays against a 100-point tree: a workgroup per ray, beyond 65 535"""
    rng = np.random.default_rng(77)
    pts = synth.uniform_cloud(100, 1.0, 78)
    t = kdtree.New(pts)
    nr = 70_000
    o = rng.uniform(-1, 2, (nr, 3)).astype(f32)
    d = (pts[rng.integers(0, 100, nr)] + rng.normal(scale=0.05, size=(nr, 3)).astype(f32)) - o
    ids = _check(t, pts, o, d, 0.05, what="70k")[0]
    assert (ids[65_536:] >= 0).sum() > 1000 and (ids < 0).sum() > 1000


# ------------------------------------------------------------------------------------------------ 8. fat rows

def test_rays_through_fat_grid_rows(monkeypatch):
    """The heap scene of tests/test_gpu_radius_edges.py: heaps of 4095, 4096, 4097 and 6000 coincident points, each a
    grid row of its own that the wave shares out.  Rays through the heaps: every heap member is counted once per ray,
    and the first hit is the heap's smallest id."""
    pts = _heap_scene()
    centres = np.array([h for h, _ in HEAPS], f64)
    rng = np.random.default_rng(6)
    o, d, s_min, s_max = [], [], [], []
    for c in centres:  # through each heap along the axes and two slants, from both sides, a window round the heap:
        for v in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0.5, 0.25], [-0.3, 1, -0.6]):  # no other point is that near it
            v = np.array(v, f64)
            o += [c - 3 * v, c + 2.5 * v]
            d += [v, -2 * v]
            s_min += [2.99, 1.24]
            s_max += [3.01, 1.26]
    for a in range(4):  # through two heaps at once, and whatever lies before, between and behind them
        for b in range(a + 1, 4):
            v = centres[b] - centres[a]
            o.append(centres[a] - v)
            d.append(v)
    o = np.concatenate([np.array(o), rng.uniform(0, 16, (40, 3)) * [1, 1, 0.25]]).astype(f32)  # and through the slab
    d = np.concatenate([np.array(d), rng.normal(size=(40, 3))]).astype(f32)
    s_min = np.concatenate([s_min, np.zeros(46)]).astype(f32)
    s_max = np.concatenate([s_max, np.full(46, inf)]).astype(f32)
    heap_ids = [np.nonzero(np.all(pts == h, axis=1))[0] for h, _ in HEAPS]
    ref = RO.query(pts, o, d, 0.05, s_min, s_max)
    for what, t, dl in _handles(pts, monkeypatch, deleted=_heap_deleted(pts)):
        ids, along, off, counts = _check(t, pts, o, d, 0.05, s_min, s_max, deleted=dl, what=what,
                                         ref=ref if dl is None else None)
        for k, h in enumerate(heap_ids):
            live = h if dl is None else np.setdiff1d(h, dl)
            assert len(np.unique(counts[live])) == 1 and counts[live[0]] >= 10, (what, k)  # 10 of its own rays, and pairs
            assert np.all(ids[10 * k:10 * k + 10] == live.min()), (what, k)


# ------------------------------------------------------------------------------------------------ 9. the device forms

def test_device_forms_and_the_carving_chain():
    import torch
    dev = torch.device("cuda", 0)
    pts = synth.surface_cloud(20_000, 5.0, 33)[0]
    n, rho = len(pts), 0.04
    t = kdtree.New(pts)
    o1, d1 = _surface_rays(1500, 21)
    o2, d2 = _surface_rays(900, 22)
    s_max = np.full(1500, 0.97, f32)
    want = t.RayCast(o1, d1, rho, None, s_max)
    c1, c2 = t.RayPierce(o1, d1, rho, None, s_max), t.RayPierce(o2, d2, rho)
    assert (want[0] >= 0).any() and c1.any() and c2.any()

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    do1, dd1, do2, dd2, dmax = up(o1), up(d1), up(o2), up(d2), up(s_max)
    di = torch.full((1500,), -7, dtype=torch.int32, device=dev)
    di2 = torch.full((1500,), -7, dtype=torch.int32, device=dev)
    da = torch.full((1500,), -7.0, dtype=torch.float64, device=dev)
    df = torch.full((1500,), -7.0, dtype=torch.float64, device=dev)
    twice = torch.zeros((n,), dtype=torch.int32, device=dev)
    both = torch.zeros((n,), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        t.RayCastDev(do1.data_ptr(), dd1.data_ptr(), 1500, rho, di.data_ptr(), da.data_ptr(), df.data_ptr(),
                     d_s_max=dmax.data_ptr(), stream=st)
        t.RayCastDev(do1.data_ptr(), dd1.data_ptr(), 1500, rho, di2.data_ptr(), d_s_max=dmax.data_ptr(), stream=st)
        for _ in range(2):
            t.RayPierceDev(do1.data_ptr(), dd1.data_ptr(), 1500, rho, twice.data_ptr(), d_s_max=dmax.data_ptr(), stream=st)
        t.RayPierceDev(do1.data_ptr(), dd1.data_ptr(), 1500, rho, both.data_ptr(), d_s_max=dmax.data_ptr(), stream=st)
        t.RayPierceDev(do2.data_ptr(), dd2.data_ptr(), 900, rho, both.data_ptr(), stream=st)
        doomed = torch.nonzero(both >= 2).flatten()  # a threshold in torch, on the same stream
        stream.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(di.cpu().numpy(), want[0]) and np.array_equal(di2.cpu().numpy(), want[0])
    assert np.array_equal(da.cpu().numpy(), want[1]) and np.array_equal(df.cpu().numpy(), want[2])
    assert np.array_equal(twice.cpu().numpy(), 2 * c1)
    assert np.array_equal(both.cpu().numpy(), c1 + c2)
    # the chain: pierced counts -> a threshold -> DeletePoints -> RayCast on the thinned set
    gone = doomed.cpu().numpy().astype(np.int64)
    assert np.array_equal(gone, np.nonzero(RO.pierce(pts, o1, d1, rho, None, s_max) + RO.pierce(pts, o2, d2, rho) >= 2)[0])
    assert 0 < len(gone) < n
    t.DeletePoints(gone)
    got = t.RayCast(o2, d2, rho)
    assert all(np.array_equal(a, b) for a, b in zip(got, RO.raycast(pts, o2, d2, rho, deleted=gone)))


# ------------------------------------------------------------------------------------------------ 10. the small tasks

def test_visible_points_of_a_sphere():
    pts = RS.sphere()
    vp = f32(RS.SPHERE_VIEW).reshape(1, 3)
    want = np.nonzero(RO.raycast(pts, np.broadcast_to(vp, pts.shape), pts - vp, RS.SPHERE_RADIUS, 0.0,
                                 f32(1.0) - f32(RS.SPHERE_SLACK))[0] < 0)[0]
    near = pts.astype(f64) @ vp[0].astype(f64) > 1.0  # (tests/test_rays_oracle.py: the same by the oracle alone)
    assert near[want].all() and 3 * len(want) >= near.sum()
    seen = rays.Visible(kdtree.New(pts), RS.SPHERE_VIEW, RS.SPHERE_RADIUS, RS.SPHERE_SLACK)
    assert seen.dtype == np.int64 and np.array_equal(seen, want)


def _wall(n=6000, seed=3):
    """a wall in the plane x = 10, 8 wide and 4 high"""
    rng = np.random.default_rng(seed)
    return np.stack([np.full(n, 10.0), rng.uniform(-4, 4, n), rng.uniform(-2, 2, n)], axis=1).astype(f32)


def test_range_image_of_a_wall():
    pts = _wall()
    az, el = np.linspace(-0.3, 0.3, 48), np.linspace(-0.15, 0.15, 12)  # inside the wall's outline
    rho = 0.08
    depth, ids = rays.RangeImage(kdtree.New(pts), (0, 0, 0), az, el, rho)
    o, d = rays.spherical_rays((0, 0, 0), az, el)
    assert o.shape == d.shape == (12 * 48, 3) and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6)
    wi, wa, _ = RO.raycast(pts, o, d, rho)
    d64 = d.astype(f64)
    dd = (d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]) + d64[:, 2] * d64[:, 2]
    assert np.array_equal(ids, wi.reshape(12, 48))
    assert np.array_equal(depth, np.where(wi >= 0, wa / np.sqrt(dd), inf).reshape(12, 48))
    hit = ids >= 0
    x = depth * np.cos(el)[:, None] * np.cos(az)[None, :]  # the hit's foot on the ray lies in the wall's plane
    assert hit.mean() > 0.9 and np.all(np.abs(x[hit] - 10.0) < 0.2)
    far = rays.RangeImage(kdtree.New(pts), (0, 0, 0), az + np.pi, el, rho)  # looking the other way
    assert np.all(np.isinf(far[0])) and np.all(far[1] == -1)


def test_see_through_a_ghost():
    """a wall, a blob in front of it that was only there for a while, and beams that end on the wall: exactly the
    blob's points were passed through"""
    rng = np.random.default_rng(14)
    wall = _wall()
    blob = (rng.normal(scale=0.15, size=(400, 3)) + [5.0, 0.5, 0.2]).astype(f32)
    pts = np.ascontiguousarray(np.concatenate([wall, blob]))
    rho, margin = 0.1, 0.02  # the beams stop 0.2 short of the wall
    # a dense fan of beams over the blob's silhouette, each ending on the wall
    y, z = np.meshgrid(np.linspace(-0.6, 2.6, 60), np.linspace(-1.0, 1.8, 50))
    ends = np.stack([np.full(y.size, 10.0), y.ravel(), z.ravel()], axis=1).astype(f32)
    origin = f32([[0, 0, 0]])
    t = kdtree.New(pts)
    counts = rays.SeeThrough(t, origin, ends, rho, margin)
    o = np.ascontiguousarray(np.broadcast_to(origin, ends.shape))
    assert np.array_equal(counts, RO.pierce(pts, o, ends - o, rho, 0.0, f32(1.0) - f32(margin)))
    assert np.array_equal(np.nonzero(counts)[0], np.arange(len(wall), len(pts)))  # exactly the blob
    t.DeletePoints(np.nonzero(counts >= 1)[0])  # the idiom of the docstring
    assert t.LiveCount() == len(wall)
