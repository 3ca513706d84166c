"""GPU: density clustering (csrc/dbscan.hip over csrc/cluster.hip; include/pcgx.h, "density clusters") against
tests/dbscan_oracle.py.  Every output is compared exactly -- labels, the count, the sizes with their zero padding, the
grouped ids with their -1 padding, kind -- at each call site, and a second call must give the same bits.
tests/test_dbscan_oracle.py pins what each scene is for."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import kdtree, segmentation, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as CO  # noqa: E402
import dbscan_oracle as DO  # noqa: E402
from dbscan_scenes import cached, chain, lattice, seven_points, uniform  # noqa: E402
from test_gpu_clusters import _deleted_ids  # noqa: E402
from test_gpu_radius_edges import HEAPS, _grid_on, _handles, _heap_scene  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
nan, inf = np.nan, np.inf


def _call(t, r, min_pts, min_size=1, max_size=0, want=(True, True, True)):
    n = t.Len()
    labels, sizes, ids = (np.full(n, -7, np.int64) for _ in range(3))
    kind = np.full(n, 77, np.uint8)
    cnt = C.c_int64(-7)
    L.check(L.lib().pcgx_kdtree_dbscan(t._h, float(r), int(min_pts), int(min_size), int(max_size), L.ptr(labels), C.byref(cnt),
                                       L.ptr(sizes) if want[0] else None, L.ptr(ids) if want[1] else None,
                                       L.ptr(kind) if want[2] else None))
    return labels, cnt.value, sizes, ids, kind


def _raw(t, r, min_pts, min_size=1, max_size=0):
    """the host entry point's whole output (labels [n], C, sizes [n], ids [n], kind [n]); a second call gives the same bits"""
    a = _call(t, r, min_pts, min_size, max_size)
    b = _call(t, r, min_pts, min_size, max_size)
    assert a[1] == b[1] and all(np.array_equal(a[k], b[k]) for k in (0, 2, 3, 4))
    return a


def _check(got, want, what):
    """exact equality with the oracle's (labels, C, sizes, ids, kind), and the padding convention said out loud"""
    labels, c, sizes, ids, kind = got
    assert np.array_equal(kind, want[4]), (what, int(np.sum(kind != want[4])))
    assert c == want[1], (what, c, want[1])
    assert np.array_equal(labels, want[0]), (what, int(np.sum(labels != want[0])))
    assert np.array_equal(sizes, want[2]), what
    assert np.array_equal(ids, want[3]), what
    total = int(sizes[:c].sum())
    assert np.all(sizes[:c] >= 1) and not sizes[c:].any(), what           # zeros behind the C sizes
    assert np.all(ids[:total] >= 0) and np.all(ids[total:] == -1), what   # -1 behind the members
    assert total == int(np.sum(labels >= 0)), what
    assert np.all(np.diff(sizes[:c]) <= 0), what                          # largest first
    assert np.all(kind[labels >= 0] > 0) and kind.max(initial=0) <= 2, what  # no noise point in a cluster


def _want(key, pts, r, min_pts, min_size=1, max_size=0):
    a = cached(("analysis", key, float(f32(r)), min_pts), lambda: DO.analyse(pts, r, min_pts))
    return CO.rank_and_group(len(pts), a["name"], min_size, max_size) + (a["kind"],)


def _cut_cloud():
    def make():
        cut = uniform().copy()
        cut[_deleted_ids(len(cut))] = nan  # the oracle's deleted point: nobody's neighbour, not even its own
        return cut
    return cached("uniform-deleted", make)


def _clusters_raw(t, r):
    n = t.Len()
    labels, sizes, ids = (np.full(n, -7, np.int64) for _ in range(3))
    cnt = C.c_int64(-7)
    L.check(L.lib().pcgx_kdtree_clusters(t._h, float(r), None, 0.0, 0, None, 0.0, 1, 0, L.ptr(labels), C.byref(cnt),
                                         L.ptr(sizes), L.ptr(ids)))
    return labels, cnt.value, sizes, ids


# ------------------------------------------------------------------------------------------------ 1. every source

@pytest.mark.parametrize("min_pts", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("r", [0.032, 0.028])
def test_every_source(r, min_pts, monkeypatch):
    pts = uniform()
    n = len(pts)
    want = _want("uniform", pts, r, min_pts)
    t = kdtree.New(pts)
    assert _grid_on(t)[3] == 1
    _check(_raw(t, r, min_pts), want, ("grid", r, min_pts))
    labels, sizes, ids, kind = t.DBSCAN(r, min_pts)  # the binding: trimmed
    total = int(want[2].sum())
    assert np.array_equal(labels, want[0]) and np.array_equal(sizes, want[2][:want[1]])
    assert np.array_equal(ids, want[3][:total]) and np.array_equal(kind, want[4])
    monkeypatch.setenv("PCGX_DBSCAN_COUNT_ALL", "1")  # the flag pass without its early stop: the same flags
    _check(_raw(t, r, min_pts), want, ("grid, whole counts", r, min_pts))
    monkeypatch.delenv("PCGX_DBSCAN_COUNT_ALL")
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    _check(_raw(t, r, min_pts), want, ("walk", r, min_pts))
    monkeypatch.delenv("PCGX_RANGE_WALK")
    gone = _deleted_ids(n)
    want_d = _want("uniform-deleted", _cut_cloud(), r, min_pts)
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    got = _raw(td, r, min_pts)
    _check(got, want_d, ("deleted", r, min_pts))
    assert np.all(got[0][gone] == -1) and not np.isin(got[3], gone).any() and not got[4][gone].any()


@pytest.mark.parametrize("r", [0.032, 0.028])
def test_min_pts_one_is_clusters(r, monkeypatch):
    """device against device: the four outputs of DBSCAN at min_pts = 1 are those of Clusters on that handle"""
    pts = uniform()
    t = kdtree.New(pts)
    td = kdtree.New(pts)
    td.DeletePoints(_deleted_ids(len(pts)))

    def both(h, what):
        a, b = _raw(h, r, 1), _clusters_raw(h, r)
        assert a[1] == b[1] and all(np.array_equal(a[k], b[k]) for k in (0, 2, 3)), what
        assert np.array_equal(a[4], np.where(a[0] >= 0, 2, 0)), what  # every usable point is core and in a cluster
    both(t, "grid")
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    both(t, "walk")
    monkeypatch.delenv("PCGX_RANGE_WALK")
    both(td, "deleted")


# ------------------------------------------------------------------------------------------------ 2. size limits

def test_size_limits():
    pts, r, min_pts = uniform(), 0.032, 4
    t = kdtree.New(pts)
    full = _want("uniform", pts, r, min_pts)
    # sizes 4, 5 and 6 occur (261, 126 and 92 times), none below 2: each limit sits at a size that occurs, or beside one
    assert full[2][0] == 377 and np.bincount(full[2][:full[1]])[:7].tolist() == [0, 0, 3, 45, 261, 126, 92]
    counts = {}
    for lo, hi in [(0, 0), (4, 0), (5, 0), (6, 0), (1, 4), (1, 5), (5, 5), (5, 6), (377, 377), (376, 378), (378, 0), (1, 1)]:
        want = _want("uniform", pts, r, min_pts, lo, hi)
        got = _raw(t, r, min_pts, lo, hi)
        _check(got, want, (lo, hi))
        assert np.array_equal(got[4], full[4])  # kind does not depend on the size range
        counts[(lo, hi)] = want[1]
    assert counts[(0, 0)] == 1104 and counts[(377, 377)] == 1 == counts[(376, 378)] and counts[(378, 0)] == 0
    assert counts[(5, 5)] == 126 and counts[(5, 6)] == 218 and counts[(1, 4)] == 309 and counts[(1, 1)] == 0
    assert counts[(4, 0)] == 1104 - 48 and counts[(5, 0)] == 1104 - 309
    dropped = _want("uniform", pts, r, min_pts, 5, 0)
    assert np.any((dropped[0] == -1) & (full[4] == 2))  # a core point of a dropped cluster: kind 2, label -1


# ------------------------------------------------------------------------------------------------ 3. ties

@pytest.mark.parametrize("swap", [False, True])
def test_seven_points(swap, monkeypatch):
    pts = seven_points(swap)
    t = kdtree.New(pts)
    want = DO.dbscan(pts, 1.0, 4)
    assert want[0].tolist() == ([0, 1, 1, 0, 0, 1, 0] if swap else [0, 0, 0, 0, 1, 1, 1])
    _check(_raw(t, 1.0, 4), want, "seven")
    _check(_raw(t, 1.0, 3), DO.dbscan(pts, 1.0, 3), "seven, all core")
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    _check(_raw(t, 1.0, 4), want, "seven, walk")


@pytest.mark.parametrize("reverse", [False, True])
def test_lattice_ties(reverse, monkeypatch):
    pts = np.ascontiguousarray(lattice()[::-1]) if reverse else lattice()
    r = 1.5 / 16
    t = kdtree.New(pts)
    td = kdtree.New(pts)
    gone = np.arange(0, len(pts), 9)
    td.DeletePoints(gone)
    cut = pts.copy()
    cut[gone] = nan
    for min_pts in (4, 5, 6):
        a = DO.analyse(pts, r, min_pts)
        assert int(a["tied"].sum()) >= (10 if min_pts == 5 else 1)
        want = CO.rank_and_group(len(pts), a["name"]) + (a["kind"],)
        _check(_raw(t, r, min_pts), want, ("lattice", reverse, min_pts))
        monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        _check(_raw(t, r, min_pts), want, ("lattice, walk", reverse, min_pts))
        monkeypatch.delenv("PCGX_RANGE_WALK")
        _check(_raw(td, r, min_pts), DO.dbscan(cut, r, min_pts), ("lattice, deleted", reverse, min_pts))


# ------------------------------------------------------------------------------------------------ 4. the chain

def test_the_chain(monkeypatch):
    """a hook chain as long as the cloud, whole and cut into 50 pieces with a border point at both ends of every piece"""
    n = 50_000
    pts, pos = chain()
    t = kdtree.New(pts)
    print("chain: grid on =", _grid_on(t)[3])
    ar = np.arange(n)
    sizes = np.zeros(n, np.int64)
    sizes[0] = n
    kind = np.full(n, 2, np.uint8)
    kind[(pos == 0) | (pos == n - 1)] = 1
    _check(_raw(t, 0.3, 3), (np.zeros(n, np.int64), 1, sizes, ar, kind), "one cluster")
    none = (np.full(n, -1), 0, np.zeros(n, np.int64), np.full(n, -1), np.zeros(n, np.uint8))
    _check(_raw(t, 0.3, 4), none, "all noise")
    _check(_raw(t, 0.25, 2), none, "DistSq == r^2 is no neighbour")
    _check(_raw(t, 0.25, 1), (ar, n, np.ones(n, np.int64), ar, np.full(n, 2, np.uint8)), "singletons")
    # cut: the handle has seen DeletePoints (the walk's form) ...
    cut, _ = chain(cut=True)
    gone = np.nonzero(pos % 1000 == 999)[0]
    want = cached("chain-cut", lambda: DO.dbscan(cut, 0.3, 3))
    assert want[1] == 50 and int(np.sum(want[4] == 1)) == 100 and int(np.sum(want[4] == 0)) == 50
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    _check(_raw(td, 0.3, 3), want, "cut, deleted")
    # ... and a handle over the remaining points (the grid's form where it has one): the same pieces under other ids
    keep = np.ones(n, bool)
    keep[gone] = False
    t2 = kdtree.New(np.ascontiguousarray(pts[keep]))
    print("cut chain: grid on =", _grid_on(t2)[3])
    new_id = np.cumsum(keep) - 1
    name = cached("chain-cut-name", lambda: DO.analyse(cut, 0.3, 3)["name"])
    # (the smallest id of a piece is the smallest new id too: the renumbering keeps the order)
    want2 = CO.rank_and_group(int(keep.sum()), new_id[name[keep]]) + (want[4][keep],)
    _check(_raw(t2, 0.3, 3), want2, "cut, rebuilt")


# ------------------------------------------------------------------------------------------------ 5. coincident heaps

def test_coincident_heaps(monkeypatch):
    """rows of thousands of records without a fat-row path: at min_pts = the smallest heap's own count the heap is all
    core, one above it is all noise unless a larger neighbour rescues it"""
    pts = cached("heaps", lambda: _heap_scene(10_000))
    r = 0.5
    heap_ids = [np.nonzero(np.all(pts == h, axis=1))[0] for h, _ in HEAPS]
    assert [len(i) for i in heap_ids] == [4095, 4096, 4097, 6000]
    own = int(DO.analyse(pts, r, 1)["count"][heap_ids[0][0]])
    assert own >= 4095
    wants = {m: cached(("heaps", m), lambda m=m: DO.dbscan(pts, r, m)) for m in (own, own + 1)}
    assert np.all(wants[own][4][heap_ids[0]] == 2) and np.all(wants[own + 1][4][heap_ids[0]] < 2)
    assert np.all(wants[own + 1][4][heap_ids[3]] == 2)
    for name, t, _ in _handles(pts, monkeypatch, rows=False):
        for m in (own, own + 1):
            _check(_raw(t, r, m), wants[m], (name, m))


# ------------------------------------------------------------------------------------------------ 6. edges of the contract

def test_small_and_degenerate_clouds():
    one = kdtree.New(f32([[1, 2, 3]]))
    _check(_raw(one, 0.1, 1), (np.array([0]), 1, np.array([1]), np.array([0]), np.array([2], np.uint8)), "Len() 1")
    _check(_raw(one, 0.1, 2), (np.array([-1]), 0, np.array([0]), np.array([-1]), np.array([0], np.uint8)), "Len() 1, noise")
    _check(_raw(one, 0.1, 1, 2), (np.array([-1]), 0, np.array([0]), np.array([-1]), np.array([2], np.uint8)), "Len() 1, small")
    for n in (2, 63, 64, 65, 257):
        rng = np.random.default_rng(100 + n)
        pts = (rng.integers(0, 6, (n, 3)) / 8.0).astype(f32)
        t = kdtree.New(pts)
        for r in (0.125, 0.13, 0.3):
            for min_pts in (1, 2, 3, 5):
                _check(_raw(t, r, min_pts), DO.dbscan(pts, r, min_pts), (n, r, min_pts))
    # NaN points only
    n = 100
    t = kdtree.New(np.full((n, 3), nan, f32))
    none = (np.full(n, -1), 0, np.zeros(n, np.int64), np.full(n, -1), np.zeros(n, np.uint8))
    _check(_raw(t, 0.5, 1), none, "NaN cloud")
    _check(_raw(t, 0.5, 3), none, "NaN cloud, min_pts 3")
    pts = synth.uniform_cloud(1000, 1.0, 75)
    # infinite coordinates among finite ones: unusable, and nobody's neighbour
    pts2 = pts.copy()
    pts2[3::11, 1] = inf
    pts2[5::13, 2] = -inf
    for min_pts in (1, 3):
        want = DO.dbscan(pts2, 0.1, min_pts)
        assert not want[4][3::11].any() and not want[4][5::13].any() and want[1] > 1
        _check(_raw(kdtree.New(pts2), 0.1, min_pts), want, ("inf points", min_pts))
    # NaN coordinates among finite ones: the neighbourhoods are Range's on that handle, whose tree a NaN puts out of
    # order, so no brute force says what they are -- but a NaN point is never usable, and the outputs agree with each other
    pts3 = pts.copy()
    pts3[::7] = nan
    labels, c, sizes, ids, kind = _raw(kdtree.New(pts3), 0.1, 3)
    assert not kind[::7].any() and np.all(labels[::7] == -1)
    assert np.array_equal(labels >= 0, kind > 0)
    assert np.array_equal(np.bincount(labels[labels >= 0], minlength=1000), sizes) and c == int(np.sum(sizes > 0))
    members = np.nonzero(labels >= 0)[0]
    assert np.array_equal(ids[:len(members)], members[np.argsort(labels[members], kind="stable")])
    assert np.all(ids[len(members):] == -1) and np.all(np.diff(sizes[:c]) <= 0)
    # every point deleted
    td = kdtree.New(pts)
    td.DeletePoints(np.arange(1000))
    none = (np.full(1000, -1), 0, np.zeros(1000, np.int64), np.full(1000, -1), np.zeros(1000, np.uint8))
    _check(_raw(td, 0.1, 1), none, "all deleted")
    _check(_raw(td, 0.1, 3), none, "all deleted, min_pts 3")


def test_each_optional_output_left_out():
    pts = synth.uniform_cloud(3000, 1.0, 76)
    t = kdtree.New(pts)
    for min_pts in (1, 3):
        want = DO.dbscan(pts, 0.06, min_pts, 2)
        for w in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            labels, c, sizes, ids, kind = _call(t, 0.06, min_pts, 2, 0, w)
            assert c == want[1] and np.array_equal(labels, want[0])
            assert np.array_equal(sizes, want[2]) if w[0] else np.all(sizes == -7)
            assert np.array_equal(ids, want[3]) if w[1] else np.all(ids == -7)
            assert np.array_equal(kind, want[4]) if w[2] else np.all(kind == 77)


def test_bad_arguments():
    lib = L.lib()
    pts = synth.uniform_cloud(100, 1.0, 90)
    t = kdtree.New(pts)
    lab, siz, ids = (np.full(100, -7, np.int64) for _ in range(3))
    kind = np.full(100, 77, np.uint8)
    lab32 = np.full(100, -7, np.int32)
    cnt = C.c_int64(5)
    E = L.PCGX_E_INVALID

    def call(h=t._h, r=0.1, m=3, lo=1, hi=0, labels=lab, count=C.byref(cnt)):
        return lib.pcgx_kdtree_dbscan(h, r, m, lo, hi, None if labels is None else L.ptr(labels), count, L.ptr(siz),
                                      L.ptr(ids), L.ptr(kind))

    def dev(h=t._h, r=0.1, m=3, labels=L.ptr(lab32), count=L.ptr(lab32)):
        return lib.pcgx_kdtree_dbscan_dev(h, r, m, 1, 0, labels, count, None, None, None, None)

    for r in (0.0, -1.0, inf, nan):
        assert call(r=r) == E and dev(r=r) == E
    for m in (0, -1, -(2 ** 31)):
        assert call(m=m) == E and dev(m=m) == E
    assert call(lo=-1) == E and call(hi=-1) == E and call(lo=5, hi=4) == E
    assert call(h=None) == E and dev(h=None) == E
    assert call(labels=None) == E and call(count=None) == E
    assert dev(labels=None) == E and dev(count=None) == E
    # nothing was written
    assert cnt.value == 5 and all(np.all(a == -7) for a in (lab, siz, ids, lab32)) and np.all(kind == 77)
    assert call() == L.PCGX_OK and call(lo=5, hi=5) == L.PCGX_OK and call(lo=0, hi=1) == L.PCGX_OK
    assert call(m=2 ** 31 - 1) == L.PCGX_OK and cnt.value == 0 and not kind.any()


# ------------------------------------------------------------------------------------------------ 7. one stream

def test_one_stream_to_boxes_and_footprints():
    """DBSCANDev -> GroupStatsDev -> GroupHullsDev on one stream over torch tensors, nothing read back in between, equal
    to the host forms; then the same through segmentation.DBSCAN"""
    import torch
    dev = torch.device("cuda", 0)
    pts, r, min_pts, lo = uniform(), 0.032, 4, 5
    n = len(pts)
    t = kdtree.New(pts)
    want = _want("uniform", pts, r, min_pts, lo, 0)
    c = want[1]
    host = t.DBSCAN(r, min_pts, MinSize=lo)
    assert np.array_equal(host[0], want[0]) and len(host[1]) == c and np.array_equal(host[3], want[4])
    stats = t.GroupStats(host[2], host[1])
    hulls = t.GroupHulls(host[2], host[1])
    lab, cnt, siz, ids = [torch.full((k,), -7, dtype=torch.int32, device=dev) for k in (n, 1, n, n)]
    kind = torch.full((n,), 77, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    f64 = torch.float64
    g_count = torch.zeros(n, dtype=torch.int32, device=dev)
    g_aabb = torch.zeros((n, 6), dtype=torch.float32, device=dev)
    g_cen, g_cov, g_eig, g_axes, g_obb = (torch.zeros((n, k), dtype=f64, device=dev) for k in (3, 6, 3, 9, 6))
    h_sizes = torch.zeros(n, dtype=torch.int32, device=dev)
    h_ids = torch.full((n,), -7, dtype=torch.int32, device=dev)
    h_area = torch.zeros(n, dtype=f64, device=dev)
    h_rect = torch.zeros((n, 6), dtype=f64, device=dev)
    with torch.cuda.stream(s):
        t.DBSCANDev(r, min_pts, lab.data_ptr(), cnt.data_ptr(), siz.data_ptr(), ids.data_ptr(), kind.data_ptr(), MinSize=lo,
                    stream=s.cuda_stream)
        t.GroupStatsDev(ids.data_ptr(), n, siz.data_ptr(), n, cnt.data_ptr(), g_count.data_ptr(), g_aabb.data_ptr(),
                        g_cen.data_ptr(), g_cov.data_ptr(), g_eig.data_ptr(), g_axes.data_ptr(), g_obb.data_ptr(),
                        stream=s.cuda_stream)
        t.GroupHullsDev(ids.data_ptr(), n, siz.data_ptr(), n, cnt.data_ptr(), h_sizes.data_ptr(), h_ids.data_ptr(),
                        h_area.data_ptr(), h_rect.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    torch.cuda.synchronize()
    got = (lab.cpu().numpy().astype(np.int64), int(cnt.cpu()[0]), siz.cpu().numpy().astype(np.int64),
           ids.cpu().numpy().astype(np.int64), kind.cpu().numpy())
    _check(got, want, "device form")
    dev_stats = (g_count, g_aabb, g_cen, g_cov, g_eig, g_axes, g_obb)
    for a, b in zip(dev_stats, stats):
        assert np.array_equal(a.cpu().numpy()[:c].reshape(np.shape(b)), b)
    total = int(want[2].sum())
    assert np.array_equal(h_sizes.cpu().numpy()[:c], hulls[0]) and np.array_equal(h_ids.cpu().numpy()[:total], hulls[1])
    assert np.array_equal(h_area.cpu().numpy()[:c], hulls[2]) and np.array_equal(h_rect.cpu().numpy()[:c], hulls[3])
    db = segmentation.DBSCAN(t, Eps=r, MinPoints=min_pts, MinClusterSize=lo)
    parts = db.Extract()
    assert len(parts) == c and [len(p) for p in parts] == want[2][:c].tolist()
    assert np.array_equal(np.concatenate(parts), want[3][:int(want[2].sum())])
    assert np.array_equal(db.labels, want[0]) and np.array_equal(db.kind, want[4])
    for a, b in zip(db.Boxes(), stats):
        assert np.array_equal(a, b)
    for a, b in zip(db.Footprints(), hulls):
        assert np.array_equal(a, b)
    with pytest.raises(RuntimeError):
        segmentation.DBSCAN(t, Eps=r).Boxes()
