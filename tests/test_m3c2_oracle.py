"""Pins the NumPy oracle of the cylinder statistics and M3C2's finish (tests/m3c2_oracle.py) on cases whose answers are
known by construction (tests/m3c2_scenes.py): the 8 x 8 x 8 lattice with axis-parallel and slanted cylinders, dyadic
points on the side surface and the caps and one float32 outside them; its member set against the ray oracle's on unit
axes, where the two definitions coincide; the finish on numbers worked out by hand; and the end-to-end scene's shape.
No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import m3c2_oracle as MO  # noqa: E402
import m3c2_scenes as MS  # noqa: E402
import rays_oracle as RO  # noqa: E402
import rays_scenes as RS  # noqa: E402

f32, f64 = np.float32, np.float64


def test_lattice_counts_and_sums():
    pts = RS.lattice()
    for half, cores, axes, counts, sums in MS.lattice_cylinders():
        n, s, terms = MO.stats(pts, cores, axes, MS.LATTICE_RHO, half)
        assert np.array_equal(n, counts), half
        assert np.array_equal(s, sums), half
        assert not MO.sums_within_bound(s, terms)
    # deleted points leave: the cylinder along x through (3, 3, 3) loses its middle and one cap
    half, cores, axes, _, _ = MS.lattice_cylinders()[0]
    gone = [RS.lattice_id(3, 3, 3), RS.lattice_id(5, 3, 3)]
    n, s, _ = MO.stats(pts, cores[:1], axes[:1], MS.LATTICE_RHO, half, deleted=gone)
    assert n[0] == 3 and s[0, 0] == -2.0 and s[0, 1] == 6.0


def test_dyadic_side_surface_and_caps():
    p, want = MS.dyadic()
    for axis in MS.DYADIC_AXES:
        m, a = MO.members(p, np.zeros((1, 3), f32), f32([axis]), MS.DYADIC_RHO, MS.DYADIC_HALF)
        assert np.array_equal(m[0], want), axis
        assert np.array_equal(a[0], p[:, 0].astype(f64) * axis[0])  # a = p.x d.x, exactly
        n, s, _ = MO.stats(p, np.zeros((1, 3), f32), f32([axis]), MS.DYADIC_RHO, MS.DYADIC_HALF)
        x = p[want, 0].astype(f64) * axis[0]
        assert n[0] == want.sum() == 6 and s[0, 0] == x.sum() and s[0, 1] == (x * x).sum()
    dd, rrdd, lldd, usable = MO.cyl_terms(np.zeros((1, 3)), [MS.DYADIC_AXES[0]], MS.DYADIC_RHO, MS.DYADIC_HALF)
    assert dd[0] == 4.0 and rrdd[0] == 1.0 and lldd[0] == 16.0 and usable[0]
    # non-finite points and unusable cylinders
    bad = p.copy()
    bad[0, 1], bad[5, 0] = np.nan, np.inf
    assert MO.stats(bad, np.zeros((1, 3), f32), f32([MS.DYADIC_AXES[0]]), 0.5, 2.0)[0][0] == 4
    o = f32([[np.nan, 0, 0], [0, 0, 0], [0, 0, 0], [0, np.inf, 0]])
    d = f32([[1, 0, 0], [0, 0, 0], [np.nan, 0, 0], [1, 0, 0]])
    n, s, _ = MO.stats(p, o, d, 0.5, 2.0)
    assert not n.any() and not s.any()


def test_members_are_the_ray_oracles_on_unit_axes():
    """With |d| == 1 exactly, dd == 1 and s = a: a a <= L L is -L <= a <= L for a dyadic L, the ray queries' range."""
    rng = np.random.default_rng(3)
    units = f32([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0.6, 0.8, 0], [0, -0.28, 0.96]])
    d64 = units.astype(f64)  # (3-4-5 and 7-24-25 stay only if their float32 roundings still give dd == 1)
    keep = (d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]) + d64[:, 2] * d64[:, 2] == 1.0
    units = units[keep]
    assert len(units) >= 3
    pts = rng.uniform(0, 4, (3000, 3)).astype(f32)
    cores = rng.uniform(0.5, 3.5, (200, 3)).astype(f32)
    axes = units[rng.integers(0, len(units), 200)]
    for rho, half in ((0.25, 0.5), (0.5, 1.0), (0.125, 2.0)):
        m, a = MO.members(pts, cores, axes, rho, half)
        rm, ra, _ = RO.members(pts, cores, axes, np.full(200, -half, f32), np.full(200, half, f32), rho)
        assert np.array_equal(m, rm) and np.array_equal(a, ra) and m.sum() > 500
        gone = np.arange(0, 3000, 3)
        assert np.array_equal(MO.members(pts, cores, axes, rho, half, gone)[0],
                              RO.members(pts, cores, axes, np.full(200, -half, f32), np.full(200, half, f32), rho, gone)[0])


def test_finish_by_hand():
    # axis (0, 0, 2): dd = 4.  Epoch 1: a = 0, 2, 4, 6 (metric 0 .. 3, mean 1.5, sample variance 5 / 3); epoch 2 the same
    # moved by metric 1: a + 2.
    a1 = np.array([0.0, 2.0, 4.0, 6.0])
    a2 = a1 + 2.0
    s1, s2 = [[a1.sum(), (a1 * a1).sum()]], [[a2.sum(), (a2 * a2).sum()]]
    dist, lod, sig = MO.finish([[0, 0, 2]], [4], s1, [4], s2, 0.125, 4)
    var = (56.0 - 144.0 / 4.0) / 3.0 / 4.0
    assert dist[0] == 1.0 and var == 5.0 / 3.0
    assert lod[0] == 1.96 * (np.sqrt(var / 4.0 + var / 4.0) + 0.125) and sig[0] == 0
    dist, lod, sig = MO.finish([[0, 0, 2]], [4], s1, [4], [[a2.sum() + 16, ((a2 + 4) ** 2).sum()]], 0.125, 4)
    assert dist[0] == 3.0 and sig[0] == 1
    for bad in (dict(n1=[3]), dict(n2=[3]), dict(axes=[[0, 0, 0]]), dict(axes=[[np.nan, 0, 1]])):
        args = dict(axes=[[0, 0, 2]], n1=[4], n2=[4])
        args.update(bad)
        dist, lod, sig = MO.finish(args["axes"], args["n1"], s1, args["n2"], s2, 0.0, 4)
        assert np.isnan(dist[0]) and np.isnan(lod[0]) and sig[0] == 0
    # no spread and no registration error: lod = 0, and a distance of exactly 0 is not significant
    flat = [[4.0, 4.0]]
    dist, lod, sig = MO.finish([[0, 0, 1]], [4], flat, [4], flat, 0.0, 2)
    assert dist[0] == 0.0 and lod[0] == 0.0 and sig[0] == 0


def test_plane_scene_has_a_narrow_rim():
    """The end-to-end scene of tests/test_gpu_m3c2.py, by the oracle alone: cores farther than rho from the patch's rim
    see a distance of exactly 0.5 or 0, and the excluded share is at most 15 %."""
    e1, e2 = MS.plane_epochs()
    rho, half, lift = MS.PLANE_RHO, 1.0, 0.5
    cores = e1[:600]
    axes = np.tile(f32([0, 0, 1]), (len(cores), 1))
    n1, s1, _ = MO.stats(e1, cores, axes, rho, half)
    n2, s2, _ = MO.stats(e2, cores, axes, rho, half)
    dist, lod, sig = MO.finish(axes, n1, s1, n2, s2, 2.0 ** -6, 4)
    xy = cores[:, :2].astype(f64)
    to_rim = np.abs(np.maximum(np.abs(xy[:, 0] - 4.0), np.abs(xy[:, 1] - 4.0)) - 2.0)  # the patch is [2, 6)^2
    inside = (np.abs(xy - 4.0) < 2.0).all(1)
    clear = to_rim > rho
    assert (~clear).mean() <= 0.15
    assert n1.min() >= 4 and n2.min() >= 4
    assert np.all(dist[clear & inside] == lift) and sig[clear & inside].all() and (clear & inside).sum() > 50
    assert np.all(dist[clear & ~inside] == 0.0) and not sig[clear & ~inside].any() and (clear & ~inside).sum() > 200
