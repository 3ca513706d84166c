"""Pins the NumPy oracle of the ray queries (tests/rays_oracle.py) on cases whose answers are known by construction
(tests/rays_scenes.py): the 8 x 8 x 8 lattice with axis-parallel and diagonal rays, and dyadic coordinates where every
product is exact -- a point at offset exactly rho = 0.5 is a member and the next float32 above is not, a point at
exactly s_min or s_max is a member.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays_oracle as RO  # noqa: E402
import rays_scenes as RS  # noqa: E402

f32, f64 = np.float32, np.float64


def test_lattice_hits_and_counts():
    pts = RS.lattice()
    o, d, s_min, s_max, ids, along, off, counts = RS.lattice_rays()
    got = RO.raycast(pts, o, d, RS.LATTICE_RHO, s_min, s_max)
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], along) and np.array_equal(got[2], off)
    assert np.array_equal(RO.pierce(pts, o, d, RS.LATTICE_RHO, s_min, s_max), counts)
    assert counts.sum() == 3 * 8 + 8 + 8 + 8 + 2 + 3 + 16 + 5 + 8 and counts.max() == 3


def test_lattice_after_deleting_the_first_hits():
    pts = RS.lattice()
    o, d, s_min, s_max, ids, _, _, counts = RS.lattice_rays()
    gone = np.unique(ids[ids >= 0])
    second = RO.raycast(pts, o, d, RS.LATTICE_RHO, s_min, s_max, rank=1)
    after = RO.raycast(pts, o, d, RS.LATTICE_RHO, s_min, s_max, deleted=gone)
    # a ray whose second member was another ray's first hit moves on further: compare where it was not
    same = ~np.isin(second[0], gone)
    assert same.sum() >= 8 and all(np.array_equal(a[same], b[same]) for a, b in zip(second, after))
    assert second[0][0] == RS.lattice_id(1, 0, 0) and second[1][0] == 2.0
    assert second[0][9] == RS.lattice_id(0, 1, 6) and second[1][9] == 1.0 and second[2][9] == 0.25  # the tie's loser
    c = RO.pierce(pts, o, d, RS.LATTICE_RHO, s_min, s_max, deleted=gone)
    assert not c[gone].any() and np.array_equal(np.delete(c, gone), np.delete(counts, gone))


def test_dyadic_surface_and_ends():
    p, s_min, s_max, want = RS.dyadic()
    n = len(p)
    o = np.zeros((n, 3), f32)
    d = np.tile(f32(RS.DYADIC_D), (n, 1))
    m, a, cc = RO.members(p, o, d, s_min, s_max, RS.DYADIC_RHO)
    k = np.arange(n)
    assert np.array_equal(m[k, k], want)
    assert a[0, 0] == 6.0 and cc[0, 0] == 1.0 and cc[4, 4] == 2.0  # a = 2 p.x, cc = 4 (p.y^2 + p.z^2), exactly
    dd, rrdd, a_lo, a_hi, usable = RO.ray_terms(o, d, s_min, s_max, RS.DYADIC_RHO)
    assert np.all(dd == 4.0) and np.all(rrdd == 1.0) and a_lo[6] == 2.0 and a_hi[8] == 16.0 and usable.all()


def test_unusable_rays_and_points():
    nan, inf = np.nan, np.inf
    pts = np.array([[1, 0, 0], [2, 0, 0], [nan, 0, 0], [3, inf, 0]], f32)
    o = np.zeros((8, 3), f32)
    d = np.tile(f32([1, 0, 0]), (8, 1))
    s_min, s_max = np.zeros(8, f32), np.full(8, inf, f32)
    o[1, 2] = nan
    d[2] = 0
    d[3, 1] = inf
    s_min[4] = nan
    s_max[5] = nan
    s_min[6], s_max[6] = 2, 1
    s_min[7], s_max[7] = 1.5, inf
    ids, along, off = RO.raycast(pts, o, d, 0.25, s_min, s_max)
    assert list(ids) == [0, -1, -1, -1, -1, -1, -1, 1] and list(along) == [1, 0, 0, 0, 0, 0, 0, 2] and not off.any()
    assert list(RO.pierce(pts, o, d, 0.25, s_min, s_max)) == [1, 2, 0, 0]
    assert list(RO.raycast(pts, o[:1], d[:1], 0.25, deleted=[0])[0]) == [1]
    assert list(RO.raycast(np.zeros((0, 3), f32), o, d, 0.25)[0]) == [-1] * 8


def test_sphere_visibility_parameters():
    """The radius and slack tests/test_gpu_rays.py uses for rays.Visible: by the oracle alone, what is seen lies in the
    near hemisphere and is at least a third of it."""
    pts = RS.sphere()
    vp = f32(RS.SPHERE_VIEW).reshape(1, 3)
    ids = RO.raycast(pts, np.broadcast_to(vp, pts.shape), pts - vp, RS.SPHERE_RADIUS, 0.0,
                     f32(1.0) - f32(RS.SPHERE_SLACK))[0]
    seen = ids < 0
    near = pts.astype(f64) @ vp[0].astype(f64) > 1.0  # the cap a viewer at distance 6 of a unit sphere can see: z > 1/6
    assert not np.any(seen & ~near)
    assert seen.sum() * 3 >= near.sum() > 1500
