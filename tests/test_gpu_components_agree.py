"""Region growing, cluster extraction and DBSCAN take the components of one radius graph from one engine
(csrc/radius_graph.h), so on one property value they must name the same partition -- and all three the oracle's.

Points are integers 0..5 over 8 on every axis, so every DistSq is exact: at r = 0.125 a pair at exactly r is no edge (only
coincident points join), r = 0.13 joins the axis neighbours, r = 0.3 everything up to DistSq = 5/64.  One heap of
coincident points is mixed in: 70 of them (more than a wave) where the cloud holds that many, else a third of the
cloud.  The sizes straddle a wave and the walk's 64-lane block (63, 64, 65), the grid passes' 256-lane block (255, 256,
257) and the 1024-lane block of the per-root counts (2049); 1 and 2 are the smallest clouds there are.  Every case runs
on the handle as built (its grid, where it has one), under PCGX_RANGE_WALK=1, and after DeletePoints of every 7th id
(a deleted point is its own region and nobody's cluster)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as CO  # noqa: E402

f32 = np.float32
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2049)
RADII = (0.125, 0.13, 0.3)
_CACHE = {}


def _cloud(n):
    """(points, three-valued property), the same for every test of a size; never modified"""
    if n not in _CACHE:
        rng = np.random.default_rng(9000 + n)
        pts = (rng.integers(0, 6, (n, 3)) / 8.0).astype(f32)
        heap = 70 if n >= 70 else n // 3
        pts[rng.choice(n, heap, replace=False)] = f32([0.25, 0.375, 0.5])
        prop = rng.integers(0, 3, n).astype(np.uint32)
        pts.setflags(write=False)
        prop.setflags(write=False)
        _CACHE[n] = (pts, prop)
    return _CACHE[n]


def _gone(n):
    return np.arange(0, n, 7)


def _cut(pts, deleted):
    """the oracle's deleted point: NaN coordinates, nobody's neighbour"""
    if not deleted:
        return pts
    cut = pts.copy()
    cut[_gone(len(pts))] = np.nan
    return cut


def _want_regions(pts, prop, r):
    """the oracle's components over the pairs inside the bound cut to equal property value, named by smallest id"""
    with np.errstate(invalid="ignore"):
        inside = CO.dist_sq(pts[:, None, :], pts[None, :, :]) < f32(r) * f32(r)
    a, b = np.nonzero(inside & (prop[:, None] == prop[None, :]))
    return CO.components(len(pts), a, b)


def _want(n, r, deleted):
    key = ("want", n, r, deleted)
    if key not in _CACHE:
        pts, prop = _cloud(n)
        cut = _cut(pts, deleted)
        _CACHE[key] = (CO.names(cut, r), _want_regions(cut, prop, r))
    return _CACHE[key]


def _partition(labels):
    """cluster numbers -> every point's smallest fellow member, -1 where it has no cluster"""
    labels = np.asarray(labels, np.int64)
    low = np.full(len(labels) + 1, len(labels), np.int64)
    np.minimum.at(low, labels, np.arange(len(labels)))  # (label -1 lands in the spare last word)
    return np.where(labels >= 0, low[labels], -1)


@pytest.mark.parametrize("n", SIZES)
def test_oracle_side_runs(n):
    """no GPU: the two oracle routes agree with each other on one property value, a deleted point is nobody's"""
    pts, prop = _cloud(n)
    for r in RADII:
        for deleted in (False, True):
            name, regions = _want(n, r, deleted)
            cut = _cut(pts, deleted)
            one = _want_regions(cut, np.zeros(n, np.uint32), r)
            assert np.array_equal(np.where(name >= 0, name, np.arange(n)), one), (n, r, deleted)
            assert np.array_equal(name < 0, np.isnan(cut[:, 0])), (n, r, deleted)
            assert np.all(regions >= one) and np.all(prop[regions] == prop), (n, r, deleted)  # the cut only splits
    if n >= 70:  # the heap is one component at every radius, and at 0.125 nothing but coincident points joins
        name = _want(n, 0.125, False)[0]
        _, first, count = np.unique(pts, axis=0, return_index=True, return_counts=True)
        assert count.max() >= 70 and np.array_equal(np.unique(name), np.sort(first))


@pytest.mark.gpu
@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("n", SIZES)
def test_three_features_one_partition(n, r, monkeypatch):
    from pcgol_amd import kdtree, segmentation
    pts, prop = _cloud(n)
    ids = np.arange(n)
    for source in ("grid", "walk", "deleted"):
        deleted = source == "deleted"
        name, regions = _want(n, r, deleted)
        t = kdtree.New(np.array(pts))
        if deleted:
            t.DeletePoints(_gone(n))
        monkeypatch.delenv("PCGX_RANGE_WALK", raising=False)
        if source == "walk":
            monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        what = (n, r, source)
        one = segmentation.RegionGrowing(t, np.zeros(n, np.uint32)).Components(r)
        assert np.array_equal(one, np.where(name >= 0, name, ids)), what     # one property value: the oracle's names
        assert np.array_equal(_partition(t.Clusters(r)[0]), name), what      # ... the partition Clusters gives
        assert np.array_equal(_partition(t.DBSCAN(r, 1)[0]), name), what     # ... and DBSCAN with MinPts = 1
        three = segmentation.RegionGrowing(t, np.array(prop)).Components(r)
        assert np.array_equal(three, regions), what                         # three values: the cut components
        monkeypatch.delenv("PCGX_RANGE_WALK", raising=False)
