"""The device tree build (csrc/kdtree_build_gpu.hip over the radix sort of csrc/sort.hip) against the oracle, at the
sizes where its index arithmetic is ragged and on keys that separate the sort's parts.

kdtree.New builds on the device from 32 768 points; PCGX_BUILD=gpu forces that from 2 points up, PCGX_BUILD=host the
host build (csrc/kdtree_build.cpp), PCGX_BUILD_LDS=0 keeps the device build on radix passes down to the last level.
All of them must give the oracle's in-order sequence, which defines the tree; the node array the walks read
(kb_fill_bfs_kernel) is checked by asking for every point of the cloud with the grid switched off (PCGX_GRID=0), the
grid built behind the tree by asking the same questions with it.  Every comparison is exact: ids with
np.array_equal, DistSq on its uint32 view.  The clouds are tree_build_clouds.py's."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import tree_build_clouds as TC
from pcgol_amd import _lib as L
from pcgol_amd import kdtree, pc, segmentation, synth

pytestmark = pytest.mark.gpu
f32 = np.float32
u32 = np.uint32

FAR = 20.0  # a maxRange no pair of a [0, 10)^3 cloud and its jittered queries exceeds
CLOUDS = {"distinct": TC.distinct_cloud, "lattice": TC.lattice_cloud}


def _new(pts, monkeypatch, build, lds=None):
    """kdtree.New(pts) under PCGX_BUILD=build and PCGX_BUILD_LDS=lds (None: unset)"""
    for name, value in (("PCGX_BUILD", build), ("PCGX_BUILD_LDS", lds)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    return kdtree.New(pts)


def _three(pts, monkeypatch):
    """the device build, the device build without the LDS launch, the host build"""
    return {"gpu": _new(pts, monkeypatch, "gpu"), "gpu, radix all the way": _new(pts, monkeypatch, "gpu", "0"),
            "host": _new(pts, monkeypatch, "host")}


@functools.lru_cache(maxsize=None)
def _oracle(kind, n):
    """the oracle's tree of a cached cloud: built once, shared by the tests, never changed"""
    return O.KDTree(CLOUDS[kind](n))


def _assert_trees_are_the_oracles(pts, monkeypatch, o=None, what=""):
    o = O.KDTree(pts) if o is None else o
    want, depth = o.inorder(), o.max_depth()
    for name, t in _three(pts, monkeypatch).items():
        got = t.InOrder()
        assert np.array_equal(got, want), (what, name, len(pts), int(np.sum(got != want)))
        assert t.MaxDepth() == depth, (what, name)


def _same_answers(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(u32), b[1].view(u32))


def _grid_stats(t, q, max_range):
    """pcgx_debug_grid_stats, as test_gpu_grid.py reads it: [1] cells, [2] crowding * 1000, [3] grid in use"""
    import torch
    dq = torch.from_numpy(np.array(q, f32)).cuda()
    out = (C.c_int64 * 14)()
    L.check(L.lib().pcgx_debug_grid_stats(t._h, L.ptr(dq.data_ptr()), len(q), max_range, out))
    return list(out)


# ------------------------------------------------------------------ 1. the size ladder

@pytest.mark.parametrize("kind", ["distinct", "lattice"])
@pytest.mark.parametrize("n", TC.LADDER)
def test_ladder_device_build_equals_host_build_equals_oracle(n, kind, monkeypatch):
    """PCGX_BUILD=gpu, the same with PCGX_BUILD_LDS=0, and PCGX_BUILD=host: InOrder() and MaxDepth() are the
    oracle's, on distinct random points and on a 4 x 4 x 4 lattice (every split tied: stability decides), at every
    rung of TC.LADDER.  Every rung runs both clouds in all three forms (none of them needed the allowance to drop the
    random cloud's radix-only form at the two largest rungs)."""
    _assert_trees_are_the_oracles(CLOUDS[kind](n), monkeypatch, _oracle(kind, n), kind)


@pytest.mark.parametrize("kind", ["distinct", "lattice"])
@pytest.mark.parametrize("n", TC.SWITCH)
def test_default_switch_between_host_and_device_build(n, kind, monkeypatch):
    """PCGX_BUILD unset: the host build below 32 768 points, the device build from there on -- the oracle's tree
    on either side of the switch."""
    o = _oracle(kind, n)
    t = _new(CLOUDS[kind](n), monkeypatch, None)
    assert np.array_equal(t.InOrder(), o.inorder())
    assert t.MaxDepth() == o.max_depth()


# ------------------------------------------------------------------ 2. the node array

@pytest.mark.parametrize("n", TC.NODE_RUNGS)
def test_node_array_holds_every_point_and_is_what_the_walk_reads(n, monkeypatch):
    """PCGX_GRID=0: only d_nodes can answer.  Every point of a distinct cloud (every 8th at 524 289) is found by
    Nearest within 1e-3 of itself, with its own id and DistSq 0 -- no slot of kb_fill_bfs_kernel's is empty or holds
    another point.  2000 jittered queries with every point in range: the oracle's answers and the host-built handle's,
    bit for bit.  On the lattice a self-query finds a point at its place, the same id as on the host-built handle."""
    monkeypatch.setenv("PCGX_GRID", "0")
    pts = TC.distinct_cloud(n)
    sel = np.arange(0, n, 8 if n > 500_000 else 1)
    dev, host = _new(pts, monkeypatch, "gpu"), _new(pts, monkeypatch, "host")
    ids, dsq = dev.NearestBatch(pts[sel], 1e-3)
    assert np.array_equal(ids, sel), int(np.sum(ids != sel))
    assert np.array_equal(dsq.view(u32), np.zeros(len(sel), u32))
    q = TC.jittered(pts)
    a = dev.NearestBatch(q, FAR)
    assert _same_answers(a, _oracle("distinct", n).nearest_batch(q, FAR))
    assert _same_answers(a, host.NearestBatch(q, FAR))

    lat = TC.lattice_cloud(n)
    dev, host = _new(lat, monkeypatch, "gpu"), _new(lat, monkeypatch, "host")
    ids, dsq = dev.NearestBatch(lat[sel], 1e-3)
    assert np.array_equal(dsq.view(u32), np.zeros(len(sel), u32))
    assert ids.min() >= 0 and np.array_equal(lat[ids], lat[sel])
    assert _same_answers((ids, dsq), host.NearestBatch(lat[sel], 1e-3))


# ------------------------------------------------------------------ 3. the grid behind the build

def _assert_grid_equals_walk(pts, sel, monkeypatch):
    """the device-built handle's answers with its grid == the same handle's with PCGX_GRID=0; -> the grid's stats"""
    monkeypatch.delenv("PCGX_GRID", raising=False)
    t = _new(pts, monkeypatch, "gpu")
    q = TC.jittered(pts)
    with_grid = [t.NearestBatch(pts[sel], 1e-3), t.NearestBatch(q, FAR)]
    st = _grid_stats(t, q, FAR)
    assert st[3] == 1, st  # there is a grid: what follows is not walk against walk
    monkeypatch.setenv("PCGX_GRID", "0")
    assert _grid_stats(t, q, FAR)[3] == 0
    walk = [t.NearestBatch(pts[sel], 1e-3), t.NearestBatch(q, FAR)]
    assert _same_answers(with_grid[0], walk[0]) and _same_answers(with_grid[1], walk[1])
    assert np.array_equal(walk[0][0], sel)
    return st


@pytest.mark.parametrize("n", TC.GRID_RUNGS)
def test_grid_behind_the_device_build_equals_the_walk(n, monkeypatch):
    """grid_build sorts the points' cell keys (a bit count that goes with the cloud's size) right behind the device
    build, from 64 points up: self-queries and 2000 jittered queries get the walk-only answers, bit for bit."""
    _assert_grid_equals_walk(TC.distinct_cloud(n), np.arange(0, n, 8 if n > 500_000 else 1), monkeypatch)


def test_grid_of_a_flat_cloud_behind_the_device_build(monkeypatch):
    """z constant: two dimensions with an extent, one layer of cells"""
    n = 40_001
    st = _assert_grid_equals_walk(TC.flat_cloud(n), np.arange(n), monkeypatch)
    # (one layer: ~n / 1.5 cells in all; a grid over a made-up third extent would have far fewer or far more)
    assert n // 3 < st[1] < 2 * n, st


def test_grid_of_a_surface_behind_the_device_build(monkeypatch):
    """A surface crowds the cells it passes through: grid_build sorts the keys again for smaller cells (the cloud of
    test_gpu_grid.py's test_surface_cloud_forced_grid_and_default, which asserts the same of it)."""
    pts = np.ascontiguousarray(synth.surface_cloud(60_000, 10.0, 11)[0], f32)
    assert len(np.unique(pts, axis=0)) == len(pts)
    st = _assert_grid_equals_walk(pts, np.arange(len(pts)), monkeypatch)
    assert st[2] <= 6000 and st[1] > 4 * len(pts), st  # refined: more cells than the first attempt's ~n / 1.5


# ------------------------------------------------------------------ 4. keys that separate the sort's parts

SIZES = [3000, 40_000]


@pytest.mark.parametrize("digit", [0, 1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_coordinates_that_differ_in_one_byte(n, digit, monkeypatch):
    """Only one of the coordinate sort's four passes has anything to do (and the sign fold): a pass that mis-sorts its
    digit, or reads the other pass's buffers, has nothing to hide behind."""
    _assert_trees_are_the_oracles(TC.one_live_byte_cloud(n, digit), monkeypatch, what=digit)


@pytest.mark.parametrize("kind", ["ascending", "descending4", "identical"])
@pytest.mark.parametrize("n", SIZES)
def test_clouds_that_come_sorted(n, kind, monkeypatch):
    pts = TC.sorted_cloud(n, kind)
    _assert_trees_are_the_oracles(pts, monkeypatch, what=kind)
    if kind == "identical":  # every comparison is a tie: a stable build moves nothing
        for name, t in _three(pts, monkeypatch).items():
            assert np.array_equal(t.InOrder(), np.arange(n)), name


@pytest.mark.parametrize("with_ends", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_zeros_subnormals_and_the_ends_of_the_range(n, with_ends, monkeypatch):
    """-0.0 / +0.0 (equal under <), subnormals of either sign (not equal to them), FLT_MIN, 1 and -- with_ends --
    +-FLT_MAX and +-inf: ordered_bits' integer order is the host's < on all of them.  Nearest on 500 finite queries:
    the device-built and the host-built handle walk the same tree, so the same bits; without the ends (every DistSq
    finite) also the oracle's."""
    pts = TC.edge_value_cloud(n, with_ends)
    _assert_trees_are_the_oracles(pts, monkeypatch, what=with_ends)
    q = TC.finite_jittered(pts)
    dev, host = _new(pts, monkeypatch, "gpu"), _new(pts, monkeypatch, "host")
    for max_range in (2.0, 0.05):
        a = dev.NearestBatch(q, max_range)
        assert _same_answers(a, host.NearestBatch(q, max_range)), max_range
        if not with_ends:
            assert _same_answers(a, O.KDTree(pts).nearest_batch(q, max_range)), max_range


def test_strided_cloud_takes_the_packed_clouds_tree(monkeypatch):
    """16-byte records with xyz at byte offset 4: the device build starts from the handle's own packed copy
    (csrc/knn.hip, build_tree) instead of the caller's buffer."""
    n = 40_000
    pts = TC.distinct_cloud(n)
    rec = np.zeros((n, 4), f32)
    rec[:, 0] = np.arange(n, dtype=f32)  # (a field in front that is no coordinate)
    rec[:, 1:] = pts
    cloud = pc.PointCloud(pc.PointCloudHeader(["label", "x", "y", "z"], [4] * 4, [1] * 4), n, rec.view(np.uint8).reshape(-1))
    assert cloud.Stride() == 16 and cloud.xyz_offset() == 4
    packed = _new(pts, monkeypatch, "gpu").InOrder()
    want = O.KDTree(pts).inorder()
    assert np.array_equal(packed, want)
    for lds in (None, "0"):
        t = _new(cloud, monkeypatch, "gpu", lds)
        assert np.array_equal(t.InOrder(), packed), lds
        assert np.array_equal(t.Vec3At(n - 1), pts[n - 1])


# ------------------------------------------------------------------ 5. the labelled rebuild

def _assert_rebuilt_tree_is_the_oracles(t, pts, m, seed):
    """m random ids deleted: InOrder(), in the handle's ids, is the oracle's tree over the points left, and region
    growing from 5 seeds (its Range walks read the rebuilt tree's nodes and report their labels) is the oracle's BFS
    over its own patched tree, id for id."""
    n = len(pts)
    rng = np.random.default_rng(seed)
    gone = rng.choice(n, m, replace=False)
    live = np.setdiff1d(np.arange(n), gone)
    t.DeletePoints(gone)
    assert t.LiveCount() == len(live) == n - m
    assert np.array_equal(t.InOrder(), live[O.KDTree(pts[live]).inorder()])
    ot = O.KDTree(pts)
    for i in gone:
        ot.delete_point(int(i))
    labels = rng.integers(0, 3, n).astype(u32)
    rg = segmentation.RegionGrowing(t, labels)
    sizes = []
    for k in range(5):
        p = pts[live[rng.integers(len(live))]] + f32(0.01)
        exact = O.region_growing_segment(ot, labels, p, 0.2)
        assert np.array_equal(rg.Segment(p, 0.2), exact), k
        sizes.append(len(exact))
    assert max(sizes) > 1  # (regions, not single points)


def test_rebuild_after_delete_on_the_device(monkeypatch):
    """50 000 points, 10 000 deleted: the tree over the 40 000 left is built on the device with a label array
    (resolve_tree in csrc/knn.hip), PCGX_BUILD unset."""
    monkeypatch.delenv("PCGX_BUILD", raising=False)
    pts = TC.distinct_cloud(50_000, 5.5)
    _assert_rebuilt_tree_is_the_oracles(kdtree.New(pts), pts, 10_000, 50)


@pytest.mark.parametrize("lds", [None, "0"])
def test_rebuild_after_delete_on_the_device_at_a_ragged_small_size(lds, monkeypatch):
    """3000 points, 700 deleted, PCGX_BUILD=gpu: the same path with 2300 points to build over"""
    pts = TC.distinct_cloud(3000, 2.2)
    _assert_rebuilt_tree_is_the_oracles(_new(pts, monkeypatch, "gpu", lds), pts, 700, 52)
