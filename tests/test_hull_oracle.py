"""Known answers of the exact footprint oracle (tests/hull_oracle.py), the restatement of include/pcgx.h's "group
footprints" that the device tests compare with."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_oracle as HO  # noqa: E402

f32 = np.float32


def _pts(xy):
    xy = np.asarray(xy, f32).reshape(-1, 2)
    return np.concatenate([xy, np.arange(len(xy), dtype=f32)[:, None]], axis=1)  # (z plays no part)


def _one(xy, ids=None):
    P = _pts(xy)
    ids = np.arange(len(P)) if ids is None else np.asarray(ids)
    F, info = HO.group_hulls(P, ids, [len(ids)])
    return F, info, F.hull_ids[: F.hull_sizes[0]].tolist()


def test_unit_square_with_inner_boundary_and_duplicate_points():
    # centre, edge midpoints, the corner (1, 1) twice (ids 9 and 2), (0, 0) twice (ids 7 and 5)
    xy = [[0.5, 0.5], [0.5, 0], [1, 1], [1, 0.5], [0, 1], [0, 0], [0.5, 1], [0, 0], [1, 0], [1, 1], [0, 0.5]]
    F, info, v = _one(xy)
    assert F.hull_sizes.tolist() == [4] and v == [5, 8, 2, 4]  # from (0, 0) counter-clockwise, the smallest ids
    assert F.hull_ids[4:].tolist() == [-1] * 7
    assert F.area[0] == 1.0 and F.rect_area[0] == 1.0 and info["D"][0] == np.sqrt(2.0)


def test_degenerate_groups():
    F, _, v = _one([[2, 2], [0, 0], [1, 1]])
    assert F.hull_sizes.tolist() == [2] and v == [1, 0] and F.area[0] == 0 and F.rect_area[0] == 0
    F, _, v = _one([[3, -4]] * 5, ids=[4, 2, 3, 2, 4])
    assert F.hull_sizes.tolist() == [1] and v == [2]
    F, _, v = _one([[-0.0, 0.0], [0.0, -0.0], [1, 0], [-0.0, -0.0]], ids=[3, 1, 2, 0])
    assert F.hull_sizes.tolist() == [2] and v == [0, 2]  # one place for every zero, its smallest id
    F, _, v = _one(np.zeros((0, 2)))
    assert F.hull_sizes.tolist() == [0] and v == []


def test_groups_clip_and_dead_members():
    P = _pts([[0, 0], [4, 0], [4, 3], [0, 3], [2, 1], [9, 9]])
    P[5, 1] = np.nan
    ids = np.array([0, 1, 2, 3, 4, 5, -1, 7, 4, 4, 2, 3, 0])
    F, info = HO.group_hulls(P, ids, [8, 0, 2, 3, -4, 6])
    assert F.hull_sizes.tolist() == [4, 0, 1, 3, 0, 0]  # the last group is clipped away, ids 5, -1 and 7 are dead
    assert F.hull_ids.tolist() == [0, 1, 2, 3, 4, 0, 2, 3] + [-1] * 5
    assert F.area.tolist() == [12.0, 0, 0, 6.0, 0, 0] and info["D"][0] == 5.0
    F, _ = HO.group_hulls(P, ids, [8, 0, 2, 3, -4, 6], n_groups=1, cap_ids=3)
    assert F.hull_sizes.tolist() == [3, 0, 0, 0, 0, 0] and F.hull_ids.tolist() == [0, 1, 2]


def test_l_shaped_footprint_takes_its_own_bounding_rectangle():
    """An L of points, the long arm along a direction that is no coordinate axis: the minimum-area rectangle over the
    hull's edges is the L's own bounding rectangle (60 x 30 in the L's frame), smaller than the rectangle along the
    principal axes, which run near the L's diagonal."""
    arm = [(i, 0) for i in range(13)] + [(0, j) for j in range(1, 7)]  # steps of length 5 along (4, 3) and (-3, 4): exact
    xy = np.array([(4 * a - 3 * b + 10, 3 * a + 4 * b - 5) for a, b in arm], np.float64)
    F, info, v = _one(xy)
    assert F.hull_sizes[0] == 3 and v == [18, 0, 12]  # the short arm's end (the least x), the corner, the long arm's end
    assert F.rect_area[0] == 60.0 * 30.0 and F.area[0] == 900.0
    X = xy - xy.mean(axis=0)
    w, V = np.linalg.eigh(X.T @ X)
    e = X @ V
    principal = np.prod(e.max(axis=0) - e.min(axis=0))
    assert principal > 1.05 * F.rect_area[0], principal  # (1899 against 1800)


def test_exact_where_float64_is_not():
    """near-collinear points whose float64 determinant has the wrong sign (the family of tests/test_hull_terms_host.py
    at k = 30): the oracle's integers decide"""
    a = (f32(0.5) + f32(3 * 2.0 ** -24), f32(0.5) + f32(2 * 2.0 ** -24))
    b, c = (f32(12 * 2.0 ** 30),) * 2, (f32(24 * 2.0 ** 30),) * 2
    A, B, C = (tuple(HO.integers(p)) for p in (a, b, c))
    assert HO.orient(A, B, C) == -HO.orient(B, A, C) == HO.orient(B, C, A)
    want = Fraction(float(a[0])) - Fraction(float(a[1]))  # the determinant is (ax - ay) (bx - cx) up to a positive factor
    assert HO.orient(A, B, C) == (1 if (want * (float(b[0]) - float(c[0]))) > 0 else -1)
