"""The NumPy oracle of density clustering (tests/dbscan_oracle.py) on cases small enough to write down, and on the
scenes the GPU tests use: the figures asserted here say what each scene is for, so a scene cannot go vacuous."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as CO  # noqa: E402
import dbscan_oracle as DO  # noqa: E402
from dbscan_scenes import chain, lattice, seven_points, uniform  # noqa: E402

f32 = np.float32


def _counts(kind):
    return [int(np.sum(kind == k)) for k in (DO.CORE, DO.BORDER, DO.NOISE)]


def test_seven_points_on_a_line():
    pts = seven_points()
    labels, c, sizes, ids, kind = DO.dbscan(pts, 1.0, 4)
    assert kind.tolist() == [2, 1, 1, 1, 1, 2, 1]
    assert c == 2 and sizes[:2].tolist() == [4, 3] and not sizes[2:].any()
    # the point at 0 is at float32-equal DistSq from both cores: the smaller id takes it
    assert CO.dist_sq(pts[3], pts[0]) == CO.dist_sq(pts[3], pts[5])
    assert labels.tolist() == [0, 0, 0, 0, 1, 1, 1] and ids.tolist() == [0, 1, 2, 3, 4, 5, 6]
    swapped = seven_points(swap=True)
    labels, c, sizes, ids, kind = DO.dbscan(swapped, 1.0, 4)
    assert kind.tolist() == [2, 1, 1, 1, 1, 2, 1] and sizes[:2].tolist() == [4, 3]
    assert labels.tolist() == [0, 1, 1, 0, 0, 1, 0] and ids.tolist() == [0, 3, 4, 6, 1, 2, 5]
    labels, c, sizes, ids, kind = DO.dbscan(pts, 1.0, 3)
    assert np.all(kind == 2) and c == 1 and sizes[0] == 7 and not labels.any()
    # the size range cuts clusters, never kinds
    labels, c, sizes, ids, kind = DO.dbscan(pts, 1.0, 4, 4, 0)
    assert kind.tolist() == [2, 1, 1, 1, 1, 2, 1] and c == 1 and labels.tolist() == [0, 0, 0, 0, -1, -1, -1]
    assert ids.tolist() == [0, 1, 2, 3, -1, -1, -1]


def test_the_chain():
    n = 50_000
    pts, pos = chain()
    labels, c, sizes, ids, kind = DO.dbscan(pts, 0.3, 3)
    assert c == 1 and sizes[0] == n and not labels.any() and np.array_equal(ids, np.arange(n))
    ends = np.nonzero((pos == 0) | (pos == n - 1))[0]
    assert np.all(kind[ends] == 1) and _counts(kind) == [n - 2, 2, 0]
    labels, c, sizes, ids, kind = DO.dbscan(pts, 0.3, 4)
    assert c == 0 and not kind.any() and np.all(labels == -1) and not sizes.any() and np.all(ids == -1)
    labels, c, sizes, ids, kind = DO.dbscan(pts, 0.25, 2)  # DistSq == r^2 is no neighbour
    assert c == 0 and not kind.any() and np.all(labels == -1)
    labels, c, sizes, ids, kind = DO.dbscan(pts, 0.25, 1)
    assert c == n and np.all(kind == 2) and np.array_equal(labels, np.arange(n)) and np.all(sizes == 1)
    cut, pos = chain(cut=True)
    labels, c, sizes, ids, kind = DO.dbscan(cut, 0.3, 3)
    assert c == 50 and sizes[:50].tolist() == [999] * 50 and _counts(kind) == [50 * 997, 100, 50]
    assert np.all(kind[pos % 1000 == 999] == 0) and np.all(labels[pos % 1000 == 999] == -1)
    assert np.all(kind[(pos % 1000 == 0) | (pos % 1000 == 998)] == 1)


@pytest.mark.parametrize("r", [0.032, 0.028])
def test_min_pts_one_is_euclidean_clustering(r):
    pts = uniform()
    got = DO.dbscan(pts, r, 1)
    want = CO.clusters(pts, r)
    assert got[1] == want[1] and all(np.array_equal(got[k], want[k]) for k in (0, 2, 3))
    assert np.all(got[4] == 2)


UNIFORM = {2: (18427, 0, 1573, 1497, 1754), 3: (14694, 2687, 2619, 974, 1754), 4: (9920, 5143, 4937, 1104, 377),
           6: (2783, 4922, 12295, 785, 46)}


@pytest.mark.parametrize("min_pts", sorted(UNIFORM))
def test_uniform_cloud_figures(min_pts):
    pts = uniform()
    r = DO.analyse(pts, 0.032, min_pts)
    labels, c, sizes, ids = CO.rank_and_group(len(pts), r["name"])
    core, border, noise, count, largest = UNIFORM[min_pts]
    assert _counts(r["kind"]) == [core, border, noise]
    assert c == count and sizes[0] == largest
    assert int(np.sum(labels >= 0)) == core + border
    if min_pts == 2:  # a neighbour of a core point has that point in reach: it is core itself
        assert border == 0
    if min_pts == 4:  # the case the nearest rule exists for
        assert int(np.sum(r["multi"])) == 332 and int(np.sum(r["multi"])) >= 100


@pytest.mark.parametrize("min_pts", [4, 5, 6])
def test_lattice_ties(min_pts):
    """a 48 x 48 lattice with holes, r = 1.5 / 16: the 8-neighbourhood, every DistSq exact, so border points sit at
    equal distances from cores of different components and the ids decide"""
    pts = lattice()
    n = len(pts)
    r = 1.5 / 16
    a = DO.analyse(pts, r, min_pts)
    print("lattice: n", n, "min_pts", min_pts, "kinds", _counts(a["kind"]), "multi", int(a["multi"].sum()), "tied",
          int(a["tied"].sum()))
    if min_pts == 5:
        assert int(a["tied"].sum()) >= 10
    # the ids reversed: the same sets up to the tied border points
    b = DO.analyse(pts[::-1], r, min_pts)
    kb, tb = b["kind"][::-1], b["tied"][::-1]
    assert np.array_equal(a["kind"], kb) and np.array_equal(a["tied"], tb) and np.array_equal(a["multi"], b["multi"][::-1])
    # the partitions: two points that are not tied share a cluster in one order iff they do in the other
    free = np.nonzero(~a["tied"] & (a["name"] >= 0))[0]
    na, nb = a["name"][free], b["name"][::-1][free]
    assert np.all(nb >= 0)
    _, ia = np.unique(na, return_inverse=True)
    _, ib = np.unique(nb, return_inverse=True)
    pairs = np.unique(np.stack([ia.reshape(-1), ib.reshape(-1)], axis=1), axis=0)
    assert len(pairs) == len(np.unique(ia)) == len(np.unique(ib))  # a bijection between the two numberings


def test_terms():
    inf, nan = f32(np.inf), f32(np.nan)
    assert DO.beats(1.0, 5, 2.0, 1) and not DO.beats(2.0, 1, 1.0, 5)
    assert DO.beats(1.0, 1, 1.0, 2) and not DO.beats(1.0, 2, 1.0, 1) and not DO.beats(1.0, 2, 1.0, 2)
    assert DO.beats(-0.0, 1, 0.0, 2) and not DO.beats(0.0, 2, -0.0, 1)
    assert not DO.beats(nan, 0, inf, 9) and not DO.beats(1.0, 0, nan, 9) and DO.beats(1.0, 3, inf, 0xffffffff)
    assert DO.is_core(True, 4, 4) and DO.is_core(True, 5, 4) and not DO.is_core(True, 3, 4) and not DO.is_core(False, 9, 4)


def test_ror_keep():
    pts = uniform()[:5000].copy()
    pts[::100] = np.nan
    finite = np.all(np.isfinite(pts), axis=1)
    assert np.array_equal(DO.ror_keep(pts, 0.05, 1), finite)
    k4, n4 = DO.ror_keep(pts, 0.05, 4), DO.ror_keep(pts, 0.05, 4, negative=True)
    assert not np.any(k4 & n4) and np.array_equal(k4 | n4, finite) and 0 < k4.sum() < finite.sum()
