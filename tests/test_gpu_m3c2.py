"""Cylinder statistics and M3C2 on the GPU (KDTree.CylinderStats, pcgol_amd/change.py and their device forms) against
the NumPy oracle (tests/m3c2_oracle.py): counts by array_equal -- a property of the point set --, sums within
n 2^-53 sum|term| of the EXACT sum (the bound of any summation order, derived and not measured), on the grid, the forced
walk and after DeletePoints, and the same bits from a second call; the finish by array_equal against the NumPy finish of
the GPU's own sums."""
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import change, kdtree, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import m3c2_oracle as MO  # noqa: E402
import m3c2_scenes as MS  # noqa: E402
import rays_scenes as RS  # noqa: E402
from test_gpu_radius_edges import HEAPS, _grid_on, _handles, _heap_deleted, _heap_scene  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
nan, inf = np.nan, np.inf


def _stats(t, cores, axes, rho, half, what=""):
    """CylinderStats, and the same bits from a second call"""
    got = t.CylinderStats(cores, axes, rho, half)
    again = t.CylinderStats(cores, axes, rho, half)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), what
    return got


def _check(t, pts, cores, axes, rho, half, deleted=None, what="", ref=None):
    """against the oracle (ref: its answer where a test has it already) -> (counts, sums)"""
    wc, ws, terms = ref if ref is not None else MO.stats(pts, cores, axes, rho, half, deleted)
    counts, sums = _stats(t, cores, axes, rho, half, what)
    assert counts.dtype == np.int32 and sums.dtype == f64 and sums.shape == (len(wc), 2)
    assert np.array_equal(counts, wc), (what, "counts", np.nonzero(counts != wc)[0][:8])
    assert not MO.sums_within_bound(sums, terms)[:8], (what, "sums")
    return counts, sums


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
    gone = np.array([RS.lattice_id(3, 3, 3), RS.lattice_id(5, 3, 3), RS.lattice_id(0, 0, 0)])
    for what, t, dl in _handles(pts, monkeypatch, deleted=gone, rows=False):
        for half, cores, axes, counts, sums in MS.lattice_cylinders():
            got = _check(t, pts, cores, axes, MS.LATTICE_RHO, half, deleted=dl, what=(what, half))
            if dl is None:
                assert np.array_equal(got[0], counts) and np.array_equal(got[1], sums), (what, half)
            else:  # dyadic terms: any order sums exactly
                assert np.array_equal(got[1], MO.stats(pts, cores, axes, MS.LATTICE_RHO, half, dl)[1]), (what, half)
                if half == 2.0:
                    assert got[0][0] == 3 and got[1][0, 0] == -2.0 and got[1][0, 1] == 6.0 and got[0][6] == 1


# ------------------------------------------------------------------------------------------------ 2. a surface scene

def test_surface_scene_on_every_handle(monkeypatch):
    pts = synth.surface_cloud(20_000, 5.0, 33)[0]
    t = kdtree.New(pts)
    assert _grid_on(t)[3] == 1
    ids = np.random.default_rng(5).choice(len(pts), 2000, replace=False)
    normals = t.Normals(0.2)[0]
    cores, axes = np.ascontiguousarray(pts[ids]), np.ascontiguousarray(normals[ids])
    assert (np.abs(axes).sum(1) > 0).mean() > 0.99
    rho, half = 0.1, 0.5
    ref = MO.stats(pts, cores, axes, rho, half)  # (one brute force for the grid and the walk)
    counts, sums = _check(t, pts, cores, axes, rho, half, what="grid", ref=ref)
    assert counts.min() >= 1 and np.median(counts) > 10  # a core is in its own cylinder
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    _check(t, pts, cores, axes, rho, half, what="walk", ref=ref)
    monkeypatch.delenv("PCGX_RANGE_WALK")
    gone = np.unique(np.concatenate([ids[::2], np.arange(0, len(pts), 3)]))
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    after = _check(td, pts, cores, axes, rho, half, deleted=gone, what="deleted")[0]
    assert np.all(after <= counts) and after.sum() < 0.8 * counts.sum()


# ------------------------------------------------------------------------------------------------ 3. surface and caps

def test_side_surface_and_caps(monkeypatch):
    p, member = MS.dyadic()
    zero = np.zeros((1, 3), f32)
    big = _with_filler(p, 72)
    gone = np.concatenate([[0, 6], np.arange(len(p), len(big), 5)])  # a member, a point one ulp outside, and filler
    trees = [("small", kdtree.New(p), p, None)]
    trees += [(what, t, big, dl) for what, t, dl in _handles(big, monkeypatch, deleted=gone, rows=False)]
    assert [w for w, _, _, _ in trees] == ["small", "grid", "walk", "deleted"]
    for what, t, pts, dl in trees:
        if what == "walk":
            monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        live = member.copy()
        if dl is not None:
            live[dl[dl < len(p)]] = False
        for axis in MS.DYADIC_AXES:
            counts, sums = _check(t, pts, zero, f32([axis]), MS.DYADIC_RHO, MS.DYADIC_HALF, deleted=dl, what=(what, axis))
            x = p[live, 0].astype(f64) * axis[0]
            assert counts[0] == live.sum() and sums[0, 0] == x.sum() and sums[0, 1] == (x * x).sum(), (what, axis)
        monkeypatch.delenv("PCGX_RANGE_WALK", raising=False)
    for i in range(len(p)):  # a tree of one point: in or out
        one = kdtree.New(p[i:i + 1].copy())
        for axis in MS.DYADIC_AXES:
            assert one.CylinderStats(zero, f32([axis]), MS.DYADIC_RHO, MS.DYADIC_HALF)[0][0] == int(member[i]), (i, axis)


# ------------------------------------------------------------------------------------------------ 4. axis length

def test_counts_do_not_depend_on_the_axis_length(monkeypatch):
    pts = synth.surface_cloud(20_000, 5.0, 36)[0]
    rng = np.random.default_rng(6)
    cores = np.ascontiguousarray(pts[rng.choice(len(pts), 500, replace=False)])
    axes = rng.normal(size=(500, 3)).astype(f32)
    gone = np.arange(1, len(pts), 4)
    for what, t, dl in _handles(pts, monkeypatch, deleted=gone, rows=False):
        base = _stats(t, cores, axes, 0.1, 0.5, what)
        assert base[0].sum() > 3000
        for scale in (2.0, 0.5, 2.0 ** -10):  # a power of two scales every a, dd and cc exactly
            got = _stats(t, cores, axes * f32(scale), 0.1, 0.5, (what, scale))
            assert np.array_equal(got[0], base[0]), (what, scale)
            assert np.array_equal(got[1], base[1] * [scale, scale * scale]), (what, scale)
        _check(t, pts, cores[:100], axes[:100] * f32(2.0 ** -10), 0.1, 0.5, deleted=dl, what=(what, "tiny axes"))


# ------------------------------------------------------------------------------------------------ 5. slab borders, every W

@pytest.mark.parametrize("spacing", ["rho", "2rho", "h", "0.37rho"])
def test_collinear_points_on_slab_borders(spacing, monkeypatch):
    """A thousand points on the axis itself, evenly spaced: whatever the slab length, many fall on or beside slab
    borders.  Each is counted exactly once, at L / rho = 6, 14, 60 and 300: a slab bound of at most 8, 16 and 64 on the
    walks (2 rho slabs; the grid's are a cell long and fewer), and several rounds of 64."""
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
    at = np.arange(0, 1000, 37)
    cores = np.zeros((len(at) + 3, 3), f32)
    cores[:len(at), 0] = line[at, 0]
    cores[len(at):, 0] = [-1.0, 0.5 * (x[500] + x[501]), x[-1] + 0.25]  # before the line, between two points, beyond it
    cx = cores[:, 0].astype(f64)
    axes = np.tile(f32([1, 0, 0]), (len(cores), 1))
    axes[1::2] = [-3, 0, 0]
    gone = np.arange(5, 1000, 11)
    for what, t, dl in _handles(pts, monkeypatch, deleted=gone, rows=False):
        live = np.ones(1000, bool)
        if dl is not None:
            live[dl] = False
        for ratio in (6, 14, 60, 300):
            half = ratio * rho  # dyadic: a a <= L L dd is |x - core| <= L exactly
            counts = _check(t, pts, cores, axes, rho, half, deleted=dl, what=(what, ratio))[0]
            want = (np.abs(x[None, live] - cx[:, None]) <= half).sum(1)
            assert np.array_equal(counts, want), (what, ratio)


# ------------------------------------------------------------------------------------------------ 6. fat rows

def test_cylinders_through_fat_grid_rows(monkeypatch):
    """The heap scene of tests/test_gpu_radius_edges.py: heaps of 4095, 4096, 4097 and 6000 coincident points, each a
    grid row of its own that the wave shares out.  A cylinder through a heap holds every live point of it, one through
    two heaps both."""
    pts = _heap_scene()
    centres = np.array([h for h, _ in HEAPS], f64)
    cores, axes, through = [], [], []
    for k, c in enumerate(centres):  # through each heap along the axes and two slants, the core beside the heap
        for v in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0.5, 0.25], [-0.3, 1, -0.6]):
            v = np.array(v, f64)
            for off in (0.0, 0.2, -0.7):
                cores.append(c + off * v / np.linalg.norm(v))
                axes.append(v)
                through.append([k])
    for a in range(4):  # through two heaps at once, from the middle between them
        for b in range(a + 1, 4):
            cores.append(0.5 * (centres[a] + centres[b]))
            axes.append(centres[b] - centres[a])
            through.append([a, b])
    rng = np.random.default_rng(6)
    cores = np.concatenate([np.array(cores), rng.uniform(0, 16, (40, 3)) * [1, 1, 0.25]]).astype(f32)  # and in the slab
    axes = np.concatenate([np.array(axes), rng.normal(size=(40, 3))]).astype(f32)
    heap_ids = [np.nonzero(np.all(pts == h, axis=1))[0] for h, _ in HEAPS]
    rho, half = 0.05, 1.0
    ref = MO.stats(pts, cores, axes, rho, half)
    for what, t, dl in _handles(pts, monkeypatch, deleted=_heap_deleted(pts)):
        counts = _check(t, pts, cores, axes, rho, half, deleted=dl, what=what, ref=ref if dl is None else None)[0]
        sizes = [len(h if dl is None else np.setdiff1d(h, dl)) for h in heap_ids]
        for i, ks in enumerate(through):
            extra = counts[i] - sum(sizes[k] for k in ks)
            assert 0 <= extra < 200, (what, i, ks, counts[i])


def test_fat_row_in_a_later_round_on_the_grid(monkeypatch):
    """A cloud 128 long with a heap of 5000 coincident points at x = 120, and cylinders along x from the middle that
    reach both ends: on the grid a slab is a cell long, the heap's slab lies beyond the first round of 64 (asserted from
    the grid's cell edge), so the wave's share of the fat row is taken for a slab of a later round."""
    heap = f32([120, 2, 2])
    back = synth.uniform_cloud(20_000, 1.0, 23) * f32([128, 4, 4])
    pts = np.ascontiguousarray(np.concatenate([back, np.repeat(heap[None, :], 5000, axis=0)]))
    rho, half = 0.05, 64.0
    slant = np.array([1, 2.0 ** -11, 0], f64)
    cores = f32([[64, 2, 2], heap.astype(f64) - 56 * slant, [64, 2, 2], [100, 2, 2]])
    axes = f32([[1, 0, 0], slant, [-2, 0, 0], [0.5, 0, 0]])
    gone = np.concatenate([np.arange(0, 20_000, 6), np.arange(20_000, 25_000, 9)])
    for what, t, dl in _handles(pts, monkeypatch, deleted=gone, rows=False):
        if what == "grid":
            h = float(_geometry(t)[0][3])
            assert 2 * rho < h and (120.0 - 0.5) / h > 64 + 2 and 2 * half / h > 64, h  # the heap's slab: round 2 or later
        counts = _check(t, pts, cores, axes, rho, half, deleted=dl, what=what)[0]
        size = 5000 if dl is None else 5000 - len(np.arange(20_000, 25_000, 9))
        assert np.all(counts >= size) and np.all(counts < size + 300), (what, counts)


# ------------------------------------------------------------------------------------------------ 7. far off

def test_far_off_cloud(monkeypatch):
    """+4096 on every axis, rho = 2^-6: the float32 centre of a ball is 2^-12 coarse there, the cover's margin grows"""
    pts = synth.surface_cloud(20_000, 5.0, 35)[0] * f32(0.5) + f32(4096)
    rng = np.random.default_rng(8)
    ids = rng.choice(len(pts), 600, replace=False)
    cores = np.ascontiguousarray(pts[ids])
    axes = kdtree.New(pts).Normals(0.1)[0][ids]
    axes[::3] = rng.normal(size=(200, 3)).astype(f32)  # slanted ones too
    ref = MO.stats(pts, cores, axes, 2.0 ** -6, 0.125)
    gone = np.setdiff1d(np.arange(0, len(pts), 5), ids)  # (the cores stay: each is in its own cylinder)
    for what, t, dl in _handles(pts, monkeypatch, deleted=gone, rows=False):
        counts = _check(t, pts, cores, axes, 2.0 ** -6, 0.125, deleted=dl, what=what, ref=ref if dl is None else None)[0]
        assert counts.min() >= 1 and counts.mean() > (1.5 if dl is None else 1.3), what


# ------------------------------------------------------------------------------------------------ 8. the contract's edges

def _edge_cylinders():
    o = np.tile(f32([0.5, 0.5, 0.5]), (10, 1))
    d = np.tile(f32([1, 0.01, 0.02]), (10, 1))
    o[1] = [5, 5, 5]             # misses the box
    o[2, 1] = nan
    o[3, 0] = -inf
    d[4] = 0                     # dd == 0
    d[5] = [0, -0.0, 0]
    d[6, 1] = nan
    d[7, 0] = inf
    d[8] = [1e-20, 1e-22, 2e-22]  # a tiny axis
    o[9] = [-0.05, 0.5, 0.5]     # outside the box, reaching in
    return o, d


def test_contract_edges(monkeypatch):
    o, d = _edge_cylinders()
    pts = synth.uniform_cloud(4000, 1.0, 41)
    for what, t, dl in _handles(pts, monkeypatch, deleted=np.arange(0, 4000, 7), rows=False):
        counts, sums = _check(t, pts, o, d, 0.05, 0.3, deleted=dl, what=what)
        assert counts[0] > 0 and counts[8] > 0 and counts[9] > 0, what
        assert not counts[1:8].any() and not sums[1:8].any(), what
    # fewer than 64 points (no grid), NaN and infinite points among finite ones
    for n in (1, 2, 63):
        small = pts[:n].copy()
        _check(kdtree.New(small), small, o, d, 0.3, 0.6, what=n)
    bad = pts[:500].copy()
    bad[::9, 1] = nan
    bad[4::9, 0] = inf
    bad[0] = nan  # (the first point too: the build's own box starts there)
    tb = kdtree.New(bad)
    assert _check(tb, bad, o, d, 0.1, 0.4, what="nan points")[0][0] > 0
    infs = pts[:500].copy()  # infinite points only
    infs[4::9, 0] = inf
    infs[7::9, 2] = -inf
    ti = kdtree.New(infs)
    assert _check(ti, infs, o, d, 0.1, 0.4, what="inf points")[0][0] > 0
    ti.DeletePoints(np.arange(0, 500, 5))
    _check(ti, infs, o, d, 0.1, 0.4, deleted=np.arange(0, 500, 5), what="inf points, deleted")
    tb.DeletePoints(np.arange(1, 500, 5))
    _check(tb, bad, o, d, 0.1, 0.4, deleted=np.arange(1, 500, 5), what="nan points, deleted")
    allnan = np.full((70, 3), nan, f32)
    got = _check(kdtree.New(allnan), allnan, o, d, 0.1, 0.4, what="all nan")
    assert not got[0].any() and not got[1].any()
    # every point deleted
    td = kdtree.New(pts[:200].copy())
    td.DeletePoints(np.arange(200))
    got = _check(td, pts[:200], o, d, 0.3, 0.6, deleted=np.arange(200), what="all deleted")
    assert not got[0].any() and not got[1].any()
    with pytest.raises(L.ErrNoPoint):  # Len() == 0 cannot be built (the reference panics there): no empty-tree case
        kdtree.New(np.zeros((0, 3), f32))
    # m == 0
    got = kdtree.New(pts).CylinderStats(np.zeros((0, 3), f32), np.zeros((0, 3), f32), 0.1, 0.4)
    assert got[0].shape == (0,) and got[1].shape == (0, 2)
    with pytest.raises(ValueError):
        kdtree.New(pts).CylinderStats(o, d[:3], 0.1, 0.4)


def test_bad_arguments_leave_the_outputs_untouched():
    lib = L.lib()
    pts = synth.uniform_cloud(100, 1.0, 90)
    t = kdtree.New(pts)
    o, d = np.tile(f32([0.5, 0.5, 0.5]), (5, 1)), np.tile(f32([1, 0, 0]), (5, 1))
    counts, sums = np.full(5, -7, np.int32), np.full(10, -7.0)

    def host(tree=t._h, po=L.ptr(o), pd=L.ptr(d), m=5, r=0.2, h=0.4, c=L.ptr(counts), s=L.ptr(sums)):
        return lib.pcgx_kdtree_cylinder_stats(tree, po, pd, m, r, h, c, s)

    def dev(tree=t._h, po=L.ptr(o), pd=L.ptr(d), m=5, r=0.2, h=0.4, c=L.ptr(counts), s=L.ptr(sums)):
        return lib.pcgx_kdtree_cylinder_stats_dev(tree, po, pd, m, r, h, c, s, None)  # (rejected before anything is read)
    for f in (host, dev):
        for v in (0.0, -1.0, inf, nan):
            assert f(r=v) == L.PCGX_E_INVALID and f(h=v) == L.PCGX_E_INVALID
        assert f(tree=None) == L.PCGX_E_INVALID
        for name in ("po", "pd", "c", "s"):
            assert f(**{name: None}) == L.PCGX_E_INVALID
        assert f(m=-1) == L.PCGX_E_INVALID and f(m=2 ** 31) == L.PCGX_E_INVALID
        assert f(po=None, pd=None, c=None, s=None, m=0) == L.PCGX_OK  # m == 0 is fine, with nothing to point at
    wide = kdtree.New(f32([[0, 0, 0], [2.0 ** 62, 0, 0], [1, 1, 1]]))
    assert host(tree=wide._h) == L.PCGX_E_INVALID and dev(tree=wide._h) == L.PCGX_E_INVALID
    assert np.all(counts == -7) and np.all(sums == -7.0)
    n = np.full(5, 9, np.int32)
    s = np.tile([9.0, 9.5], 5)
    dist, lod, sig = np.full(5, -7.0), np.full(5, -7.0), np.full(5, 7, np.uint8)

    def fin(pa=L.ptr(d), a=L.ptr(n), b=L.ptr(s), c=L.ptr(n), e=L.ptr(s), m=5, reg=0.0, k=4, x=L.ptr(dist), y=L.ptr(lod),
            z=L.ptr(sig)):
        return lib.pcgx_m3c2_finish(pa, a, b, c, e, m, reg, k, x, y, z)

    def fin_dev(pa=L.ptr(d), a=L.ptr(n), b=L.ptr(s), c=L.ptr(n), e=L.ptr(s), m=5, reg=0.0, k=4, x=L.ptr(dist), y=L.ptr(lod),
                z=L.ptr(sig)):
        return lib.pcgx_m3c2_finish_dev(pa, a, b, c, e, m, reg, k, x, y, z, None)
    for f in (fin, fin_dev):
        assert f(m=-1) == L.PCGX_E_INVALID
        for v in (-1e-300, -1.0, nan):
            assert f(reg=v) == L.PCGX_E_INVALID
        for v in (1, 0, -3):
            assert f(k=v) == L.PCGX_E_INVALID
        for name in ("pa", "a", "b", "c", "e", "x", "y", "z"):
            assert f(**{name: None}) == L.PCGX_E_INVALID
        assert f(pa=None, a=None, b=None, c=None, e=None, x=None, y=None, z=None, m=0) == L.PCGX_OK
    assert np.all(dist == -7.0) and np.all(lod == -7.0) and np.all(sig == 7)
    L.check(fin(reg=inf))  # an infinite registration error is >= 0: nothing is significant
    assert np.all(np.isinf(lod)) and not sig.any()


# ------------------------------------------------------------------------------------------------ 9. launch indices

def _three_handles(monkeypatch, clouds, gone):
    """(name, trees, deleted ids per tree) for several clouds at once: as built, under the forced walk, and after
    DeletePoints of gone[k] from cloud k"""
    trees = [kdtree.New(c) for c in clouds]
    yield "default", trees, [None] * len(clouds)
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    yield "walk", trees, [None] * len(clouds)
    monkeypatch.delenv("PCGX_RANGE_WALK")
    deleted = [kdtree.New(c) for c in clouds]
    for t, g in zip(deleted, gone):
        t.DeletePoints(g)
    yield "deleted", deleted, list(gone)


def test_more_cylinders_than_16_bits(monkeypatch):
    """70 000 cylinders against a 100-point tree: 8 to a wave, and -- 64 lanes each -- a workgroup per cylinder, beyond
    65 535; as built, on the forced walk and after DeletePoints"""
    rng = np.random.default_rng(77)
    pts = synth.uniform_cloud(100, 1.0, 78)
    m = 70_000
    cores = (pts[rng.integers(0, 100, m)] + rng.normal(scale=0.05, size=(m, 3))).astype(f32)
    axes = rng.normal(size=(m, 3)).astype(f32)
    gone = np.arange(3, 100, 10)
    refs = {None: MO.stats(pts, cores, axes, 0.1, 0.2), "deleted": MO.stats(pts, cores, axes, 0.1, 0.2, gone)}
    for what, (t,), (dl,) in _three_handles(monkeypatch, [pts], [gone]):
        ref = refs[None if dl is None else "deleted"]
        counts = _check(t, pts, cores, axes, 0.1, 0.2, deleted=dl, what=(what, "70k"), ref=ref)[0]
        assert (counts[65_536:] > 0).sum() > 1000 and (counts == 0).sum() > 1000, what
        monkeypatch.setenv("PCGX_CYL_LANES", "64")
        _check(t, pts, cores, axes, 0.1, 0.2, deleted=dl, what=(what, "70k, 64 lanes"), ref=ref)
        monkeypatch.delenv("PCGX_CYL_LANES")


# ------------------------------------------------------------------------------------------------ 10. the device forms

def test_device_forms_and_the_chain(monkeypatch):
    import torch
    dev = torch.device("cuda", 0)
    e1 = synth.surface_cloud(20_000, 5.0, 33)[0]
    e2 = synth.surface_cloud(20_000, 5.0, 34)[0]
    e2[:, 2] += f32(0.08) * (e2[:, 0] > 2.5)  # half of it moved
    m, rho, half = 1500, 0.1, 0.5
    ids = np.random.default_rng(2).choice(len(e1), m, replace=False)
    cores, axes = np.ascontiguousarray(e1[ids]), np.ascontiguousarray(kdtree.New(e1).Normals(0.2)[0][ids])
    axes[7] = 0  # an unusable axis
    m3 = change.M3C2(rho, half, change.WithRegistrationError(0.01), change.WithMinCount(5))
    assert (m3.RegistrationError, m3.MinCount) == (0.01, 5) and change.New(rho, half).MinCount == 4

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dc, da = up(cores), up(axes)
    stream = torch.cuda.Stream()
    for what, (t1, t2), _ in _three_handles(monkeypatch, [e1, e2], [np.arange(0, 20_000, 4), np.arange(1, 20_000, 5)]):
        if what == "default":
            assert _grid_on(t1)[3] == 1 and _grid_on(t2)[3] == 1
        want = m3.Compute(t1, t2, cores, axes)
        n1, s1 = t1.CylinderStats(cores, axes, rho, half)
        n2, s2 = t2.CylinderStats(cores, axes, rho, half)
        assert np.array_equal(want[3], n1) and np.array_equal(want[4], n2), what
        dn1 = torch.full((m,), -7, dtype=torch.int32, device=dev)
        dn2 = torch.full((m,), -7, dtype=torch.int32, device=dev)
        ds1 = torch.full((2 * m,), -7.0, dtype=torch.float64, device=dev)
        ds2 = torch.full((2 * m,), -7.0, dtype=torch.float64, device=dev)
        dist = torch.full((m,), -7.0, dtype=torch.float64, device=dev)
        lod = torch.full((m,), -7.0, dtype=torch.float64, device=dev)
        sig = torch.full((m,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            m3.ComputeDev(t1, t2, dc.data_ptr(), da.data_ptr(), m, dist.data_ptr(), lod.data_ptr(), sig.data_ptr(),
                          dn1.data_ptr(), ds1.data_ptr(), dn2.data_ptr(), ds2.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
        torch.cuda.synchronize()
        g1, g2 = ds1.cpu().numpy().reshape(-1, 2), ds2.cpu().numpy().reshape(-1, 2)
        assert np.array_equal(dn1.cpu().numpy(), n1) and np.array_equal(dn2.cpu().numpy(), n2), what
        assert np.array_equal(g1, s1) and np.array_equal(g2, s2), what  # the same handle, arguments and build: the same bits
        got = dist.cpu().numpy(), lod.cpu().numpy(), sig.cpu().numpy()
        ours = MO.finish(axes, n1, g1, n2, g2, 0.01, 5)  # the NumPy finish of the GPU's own sums
        for g, w, h in zip(got, ours, want[:3]):
            assert np.array_equal(g, w, equal_nan=True) and np.array_equal(g.astype(h.dtype), h, equal_nan=True), what
        ok = ~np.isnan(got[0])
        assert np.isnan(got[0][7]) and np.isnan(got[1][7]) and got[2][7] == 0 and ok.mean() > 0.9, what
        moved = cores[:, 0] > 2.7
        assert got[2][ok & moved].mean() > 0.8 and np.abs(np.median(got[0][ok & moved])) > 0.05, what
        assert np.abs(np.median(got[0][ok & (cores[:, 0] < 2.3)])) < 0.01, what


# ------------------------------------------------------------------------------------------------ 11. end to end

def test_raised_patch_end_to_end(monkeypatch):
    """Two noise-free samplings of the plane z = 0; in epoch 2 the patch [2, 6)^2 is raised by exactly 0.5.  Every core
    farther than rho from the patch's rim sees exactly 0.5 and significance, or exactly 0 and none -- as built, on the
    forced walk and with a third of each epoch deleted."""
    e1, e2 = MS.plane_epochs()
    rho, half, lift = MS.PLANE_RHO, 1.0, 0.5
    cores = np.ascontiguousarray(e1[kdtree.New(e1).Thin(0.1)][:3000])
    axes = np.tile(f32([0, 0, 1]), (len(cores), 1))
    xy = cores[:, :2].astype(f64)
    to_rim = np.abs(np.maximum(np.abs(xy[:, 0] - 4.0), np.abs(xy[:, 1] - 4.0)) - 2.0)
    inside = (np.abs(xy - 4.0) < 2.0).all(1)
    clear = to_rim > rho
    assert (~clear).mean() <= 0.15
    assert (clear & inside).sum() > 300 and (clear & ~inside).sum() > 1000
    # a third of each epoch's points that are at least 0.5 from the plane's border: the cylinders at the border are a
    # half or a quarter full as they are, and every cylinder keeps min_count points (checked with the oracle: 8 at least)
    gone = [np.nonzero(((e[:, :2] >= 0.5) & (e[:, :2] <= 7.5)).all(1) & (np.arange(len(e)) % 3 == k))[0]
            for k, e in enumerate((e1, e2))]
    for what, (t1, t2), _ in _three_handles(monkeypatch, [e1, e2], gone):
        if what == "default":
            assert _grid_on(t1)[3] == 1 and _grid_on(t2)[3] == 1
        m3 = change.M3C2(rho, half, change.WithRegistrationError(2.0 ** -6))
        dist, lod, sig, n1, n2 = m3.Compute(t1, t2, cores, axes)
        assert sig.dtype == bool and n1.min() >= 4 and n2.min() >= 4, what
        assert np.all(dist[clear & inside] == lift) and sig[clear & inside].all(), what
        assert np.all(dist[clear & ~inside] == 0.0) and not sig[clear & ~inside].any(), what
        assert np.all(lod[clear] == 1.96 * 2.0 ** -6), what
    # the noisy scene: only against the oracle
    q1, q2 = MS.plane_epochs(noise=0.02, seeds=(3, 4))
    cores = np.ascontiguousarray(q1[:800])
    axes = np.tile(f32([0, 0, 2]), (len(cores), 1))
    gone = [np.arange(2, len(q1), 4), np.arange(0, len(q2), 5)]
    for what, (k1, k2), (d1, d2) in _three_handles(monkeypatch, [q1, q2], gone):
        got = change.M3C2(rho, half, change.WithRegistrationError(0.01)).Compute(k1, k2, cores, axes)
        w1, w2 = MO.stats(q1, cores, axes, rho, half, d1), MO.stats(q2, cores, axes, rho, half, d2)
        assert np.array_equal(got[3], w1[0]) and np.array_equal(got[4], w2[0]), what
        g1, g2 = k1.CylinderStats(cores, axes, rho, half)[1], k2.CylinderStats(cores, axes, rho, half)[1]
        assert not MO.sums_within_bound(g1, w1[2]) and not MO.sums_within_bound(g2, w2[2]), what
        ours = MO.finish(axes, got[3], g1, got[4], g2, 0.01, 4)
        assert all(np.array_equal(g.astype(w.dtype), w, equal_nan=True) for g, w in zip(got[:3], ours)), what
        want = MO.finish(axes, w1[0], w1[1], w2[0], w2[1], 0.01, 4)  # from the exact sums: the same up to their rounding
        assert np.allclose(got[0], want[0], rtol=0, atol=1e-12) and np.allclose(got[1], want[1], rtol=1e-9, atol=0), what
