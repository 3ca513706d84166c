"""The NumPy oracle of cluster extraction (tests/cluster_oracle.py) on cases small enough to write the answer down:
a path, two triangles and an isolated point, clusters of equal size in both id orders, every boundary of min_size /
max_size, and the table of normals whose dots are exactly +-0.75."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as CO  # noqa: E402

f32 = np.float32


def _pad(vals, n, fill):
    out = np.full(n, fill, np.int64)
    out[:len(vals)] = vals
    return out


def _check(got, labels, sizes, ids):
    n = len(labels)
    assert got[0].tolist() == list(labels)
    assert got[1] == len(sizes)
    assert np.array_equal(got[2], _pad(sizes, n, 0))
    assert np.array_equal(got[3], _pad(ids, n, -1))


def test_a_path_of_five_points():
    """0.25 apart on a line (exact in float32), ids shuffled: at r = 0.25 DistSq == r^2 is not below it"""
    order = [3, 0, 4, 1, 2]  # id of the k-th point along the line
    pts = np.zeros((5, 3), f32)
    pts[order, 0] = 0.25 * np.arange(5)
    _check(CO.clusters(pts, 0.25), [0, 1, 2, 3, 4], [1] * 5, [0, 1, 2, 3, 4])
    up = np.nextafter(f32(0.25), f32(1))
    _check(CO.clusters(pts, up), [0] * 5, [5], [0, 1, 2, 3, 4])
    # without the middle point (id 4): {3, 0} and {1, 2}, equal sizes, the smaller smallest id first
    cut = pts.copy()
    cut[4] = np.nan
    _check(CO.clusters(cut, up), [0, 1, 1, 0, -1], [2, 2], [0, 3, 1, 2])
    _check(CO.clusters(cut, 0.6), [0, 0, 0, 0, -1], [4], [0, 1, 2, 3])  # 0.5 apart joins across the gap


def test_two_triangles_and_an_isolated_point():
    tri = f32([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]])
    pts = np.concatenate([tri + f32([5, 0, 0]), f32([[9, 9, 9]]), tri])  # ids 0-2, 3, 4-6
    _check(CO.clusters(pts, 0.2), [0, 0, 0, 2, 1, 1, 1], [3, 3, 1], [0, 1, 2, 4, 5, 6, 3])
    _check(CO.clusters(pts, 0.2, min_size=2), [0, 0, 0, -1, 1, 1, 1], [3, 3], [0, 1, 2, 4, 5, 6])
    _check(CO.clusters(pts, 0.2, max_size=1), [-1, -1, -1, 0, -1, -1, -1], [1], [3])
    _check(CO.clusters(pts, 0.2, min_size=4), [-1] * 7, [], [])


@pytest.mark.parametrize("flip", [False, True])
def test_equal_sizes_in_both_id_orders(flip):
    """two pairs and a triple: the triple first, then the pairs by smallest member id, wherever they lie in space"""
    a = f32([[0, 0, 0], [0.1, 0, 0]])
    b = f32([[3, 0, 0], [3.1, 0, 0]])
    c = f32([[6, 0, 0], [6.1, 0, 0], [6.2, 0, 0]])
    pts = np.concatenate([b, c, a] if flip else [a, c, b])  # ids 0-1, 2-4, 5-6
    _check(CO.clusters(pts, 0.15), [1, 1, 0, 0, 0, 2, 2], [3, 2, 2], [2, 3, 4, 0, 1, 5, 6])
    # interleaved ids: {0, 6} before {1, 5} although 1 < 6
    pts = np.concatenate([a[:1], b[:1], c, b[1:], a[1:]])
    _check(CO.clusters(pts, 0.15), [1, 2, 0, 0, 0, 2, 1], [3, 2, 2], [2, 3, 4, 0, 6, 1, 5])


def test_every_boundary_of_the_size_limits():
    """components of sizes 1, 2, 3, 4 (ids in this order): each limit at a size that occurs, one below and one above"""
    pts = np.concatenate([f32([[10.0 * s + 0.1 * k, 0, 0] for k in range(s)]) for s in (1, 2, 3, 4)])
    name = CO.names(pts, 0.15)
    assert name.tolist() == [0, 1, 1, 3, 3, 3, 6, 6, 6, 6]
    kept = lambda lo, hi: CO.rank_and_group(10, name, lo, hi)[2][:CO.rank_and_group(10, name, lo, hi)[1]].tolist()  # noqa: E731
    assert kept(0, 0) == kept(1, 0) == [4, 3, 2, 1]  # min_size 0 counts as 1
    assert kept(2, 0) == [4, 3, 2] and kept(3, 0) == [4, 3] and kept(4, 0) == [4] and kept(5, 0) == []
    assert kept(1, 4) == [4, 3, 2, 1] and kept(1, 3) == [3, 2, 1] and kept(1, 2) == [2, 1] and kept(1, 1) == [1]
    assert kept(1, 5) == [4, 3, 2, 1] and kept(2, 3) == [3, 2] and kept(3, 3) == [3] and kept(2, 2) == [2]
    labels, c, sizes, ids = CO.rank_and_group(10, name, 2, 3)
    assert labels.tolist() == [-1, 1, 1, 0, 0, 0, -1, -1, -1, -1] and c == 2
    assert ids.tolist() == [3, 4, 5, 1, 2] + [-1] * 5 and sizes.tolist() == [3, 2] + [0] * 8


TABLE = f32([(1, 0, 0), (0.75, 0.5, 0), (0.75, -0.5, 0.25), (0, 1, 0), (0, 0.75, 0.5), (0, 0, 1), (-1, 0, 0), (0, 0, 0),
             (np.nan, 0, 1), (0, np.inf, 0)])


def test_the_dot_table_at_plus_and_minus_three_quarters():
    """ten coincident-free points in a row, all within reach of each other, one normal of the table each"""
    pts = np.zeros((10, 3), f32)
    pts[:, 0] = 0.01 * np.arange(10)
    d = TABLE[:7].astype(np.float64) @ TABLE[:7].astype(np.float64).T
    assert np.all(d * 16 == np.round(d * 16)) and np.sum(np.abs(d) == 0.75) >= 6  # multiples of 1/16, many exactly 0.75
    assert CO.usable(pts, 1.0, TABLE).tolist() == [True] * 7 + [False] * 3
    up = np.nextafter(f32(0.75), f32(1))
    # |c| >= 0.75: 0-1, 0-2, 0-6 (|-1|), 1-6, 2-6 (|-0.75|), 3-4 (0.75); 5 joins nobody (0.5 with 4, 0.25 with 2)
    _check(CO.clusters(pts, 1.0, TABLE, 0.75, False), [0, 0, 0, 1, 1, 2, 0, -1, -1, -1], [4, 2, 1], [0, 1, 2, 6, 3, 4, 5])
    # one float32 above 0.75 only 0-6 (|c| = 1) is left
    _check(CO.clusters(pts, 1.0, TABLE, up, False), [0, 1, 2, 3, 4, 5, 0, -1, -1, -1], [2, 1, 1, 1, 1, 1],
           [0, 6, 1, 2, 3, 4, 5])
    # oriented: -1 and -0.75 do not hold; 6 is alone
    _check(CO.clusters(pts, 1.0, TABLE, 0.75, True), [0, 0, 0, 1, 1, 2, 3, -1, -1, -1], [3, 2, 1, 1], [0, 1, 2, 3, 4, 5, 6])
    # min_cos = -1, oriented: every pair of usable points joins, the unusable ones alone are left out
    _check(CO.clusters(pts, 1.0, TABLE, -1.0, True), [0] * 7 + [-1] * 3, [7], list(range(7)))
    # curvature on top: point 1 above the limit, point 2 NaN -> 0 keeps 6 only
    cur = f32([0, 0.5, np.nan, 0, 0, 0, 0, 0, 0, 0])
    _check(CO.clusters(pts, 1.0, TABLE, 0.75, False, cur, 0.25), [0, -1, -1, 1, 1, 2, 0, -1, -1, -1], [2, 2, 1],
           [0, 6, 3, 4, 5])


def test_coincident_points_are_one_site_only_where_their_normal_agrees_with_itself():
    pts = np.zeros((6, 3), f32)
    nrm = f32([[0.5, 0, 0]] * 3 + [[1, 0, 0]] * 3)  # 0.5 . 0.5 = 0.25 < 0.75: the copies of the short normal stay apart
    _check(CO.clusters(pts, 0.1, nrm, 0.75, False), [1, 2, 3, 0, 0, 0], [3, 1, 1, 1], [3, 4, 5, 0, 1, 2])
    _check(CO.clusters(pts, 0.1, nrm, 0.25, False), [0] * 6, [6], list(range(6)))
    _check(CO.clusters(pts, 0.1), [0] * 6, [6], list(range(6)))
