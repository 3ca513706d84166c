"""GPU: cluster extraction (csrc/cluster.hip; include/pcgx.h, "clusters") against tests/cluster_oracle.py.  Every output
is compared exactly -- labels, the count, the sizes with their zero padding, the grouped ids with their -1 padding -- at
each call site, and a second call must give the same bits.  The counts quoted in the tests were computed on the CPU with
an independent restatement of the contract; asserting them keeps each scene doing what it is for."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import kdtree, segmentation, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as CO  # noqa: E402
from test_gpu_radius_edges import HEAPS, _components_reference, _grid_on, _handles, _heap_scene  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
nan, inf = np.nan, np.inf
UP = float(np.nextafter(f32(0.75), f32(1)))
TABLE = f32([(1, 0, 0), (0.75, 0.5, 0), (0.75, -0.5, 0.25), (0, 1, 0), (0, 0.75, 0.5), (0, 0, 1), (-1, 0, 0), (0, 0, 0),
             (nan, 0, 1), (0, inf, 0)])

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _cloud():
    return _cached("cloud", lambda: synth.uniform_cloud(20_000, 1.0, 71))


def _deleted_ids(n):
    return np.sort(np.random.default_rng(73).choice(n, n // 10, replace=False))


def _names(key, pts, r, **kw):
    """the oracle's components (shared by the tests that rank them differently; never modified)"""
    name = _cached(("names", key, float(f32(r))), lambda: CO.names(pts, r, **kw))
    name.setflags(write=False)
    return name


def _opt(a):
    return None if a is None else L.ptr(a)


def _call(t, r, normals, min_cos, oriented, curvature, max_curvature, min_size, max_size, want_sizes=True, want_ids=True):
    n = t.Len()
    labels, sizes, ids = (np.full(n, -7, np.int64) for _ in range(3))
    cnt = C.c_int64(-7)
    L.check(L.lib().pcgx_kdtree_clusters(t._h, float(r), _opt(normals), float(min_cos), int(oriented), _opt(curvature),
                                         float(max_curvature), int(min_size), int(max_size), L.ptr(labels), C.byref(cnt),
                                         L.ptr(sizes) if want_sizes else None, L.ptr(ids) if want_ids else None))
    return labels, cnt.value, sizes, ids


def _raw(t, r, normals=None, min_cos=0.0, oriented=False, curvature=None, max_curvature=0.0, min_size=1, max_size=0):
    """the host entry point's whole output (labels [n], C, sizes [n], ids [n]); a second call gives the same bits"""
    nrm = None if normals is None else np.ascontiguousarray(normals, f32).reshape(-1, 3)
    cur = None if curvature is None else np.ascontiguousarray(curvature, f32)
    a = _call(t, r, nrm, min_cos, oriented, cur, max_curvature, min_size, max_size)
    b = _call(t, r, nrm, min_cos, oriented, cur, max_curvature, min_size, max_size)
    assert a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[::2] + a[3:], b[::2] + b[3:]))
    return a


def _check(got, want, what):
    """exact equality with the oracle's (labels, C, sizes, ids), and the padding convention said out loud"""
    labels, c, sizes, ids = got
    assert c == want[1], (what, c, want[1])
    assert np.array_equal(labels, want[0]), (what, int(np.sum(labels != want[0])))
    assert np.array_equal(sizes, want[2]), what
    assert np.array_equal(ids, want[3]), what
    total = int(sizes[:c].sum())
    assert np.all(sizes[:c] >= 1) and not sizes[c:].any(), what           # zeros behind the C sizes
    assert np.all(ids[:total] >= 0) and np.all(ids[total:] == -1), what   # -1 behind the members
    assert total == int(np.sum(labels >= 0)), what
    assert np.all(np.diff(sizes[:c]) <= 0), what                          # largest first


# ------------------------------------------------------------------------------------------------ 1. every source

@pytest.mark.parametrize("r, count, largest", [(0.032, 3070, [1754, 1621, 616, 449, 437]), (0.028, 6718, [81])])
def test_every_source(r, count, largest, monkeypatch):
    pts = _cloud()
    n = len(pts)
    want = CO.rank_and_group(n, _names("cloud", pts, r))
    assert want[1] == count and want[2][:len(largest)].tolist() == largest
    if r == 0.032:  # heavy ties: the order by smallest id decides hundreds of numbers
        assert np.sum(want[2] >= 5) == 555 and np.sum(want[2] == 5) == 109 and np.sum(want[2] == 6) == 56
    t = kdtree.New(pts)
    assert _grid_on(t)[3] == 1
    _check(_raw(t, r), want, ("grid", r))
    labels, sizes, ids = t.Clusters(r)  # the binding: trimmed
    assert np.array_equal(labels, want[0]) and np.array_equal(sizes, want[2][:count]) and np.array_equal(ids, want[3][:n])
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    _check(_raw(t, r), want, ("walk", r))
    monkeypatch.delenv("PCGX_RANGE_WALK")
    gone = _deleted_ids(n)
    cut = pts.copy()
    cut[gone] = nan  # the oracle's deleted point: nobody's neighbour, not even its own
    want_d = CO.rank_and_group(n, _names("cloud-deleted", cut, r))
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    got = _raw(td, r)
    _check(got, want_d, ("deleted", r))
    assert np.all(got[0][gone] == -1) and not np.isin(got[3], gone).any()  # no deleted id gets a label or a slot
    assert int(np.sum(got[0] >= 0)) == n - len(gone)


# ------------------------------------------------------------------------------------------------ 2. size limits

def test_size_limits():
    pts, r = _cloud(), 0.032
    n = len(pts)
    name = _names("cloud", pts, r)
    t = kdtree.New(pts)
    kept = {}
    # sizes 5 and 6 occur (109 and 56 times), so each limit sits at a size that occurs, one below and one above
    for lo, hi in [(4, 0), (5, 0), (6, 0), (7, 0), (1, 4), (1, 5), (1, 6), (1, 7), (5, 5), (5, 6), (6, 6), (0, 0), (1, 1),
                   (0, 1), (1754, 1754), (1753, 1755), (1755, 0), (1622, 1753)]:
        want = CO.rank_and_group(n, name, lo, hi)
        _check(_raw(t, r, min_size=lo, max_size=hi), want, (lo, hi))
        kept[(lo, hi)] = want
    assert kept[(5, 0)][1] == 555
    assert kept[(5, 5)][1] == 109 and kept[(6, 6)][1] == 56 and kept[(5, 6)][1] == 165
    assert kept[(1, 1)][1] == int(np.sum(kept[(0, 0)][2] == 1)) > 0 and np.all(kept[(1, 1)][2][:kept[(1, 1)][1]] == 1)
    assert np.array_equal(kept[(1, 1)][3][:kept[(1, 1)][1]], np.sort(kept[(1, 1)][3][:kept[(1, 1)][1]]))  # singletons by id
    assert kept[(1754, 1754)][1] == 1 and kept[(1754, 1754)][2][0] == 1754
    assert kept[(1753, 1755)][1] == 1 and kept[(1755, 0)][1] == 0 and kept[(1622, 1753)][1] == 0


# ------------------------------------------------------------------------------------------------ 3. the threshold

THRESHOLD = [(0.75, False, 2776, 6805), (UP, False, 6838, 52), (0.75, True, 4672, 862), (-1.0, True, 41, 13964)]


def _table_normals(n):
    return np.ascontiguousarray(TABLE[np.random.default_rng(72).integers(0, 10, n)])


@pytest.mark.parametrize("min_cos, oriented, count, largest", THRESHOLD)
def test_the_threshold_exactly(min_cos, oriented, count, largest, monkeypatch):
    """every dot of two normals of the table is a multiple of 1/16 and many are exactly +-0.75: MinCos = 0.75 keeps
    them, its float32 successor drops them; at MinCos = -1, oriented, the 5983 unusable points alone cut the graph"""
    pts, r = _cloud(), 0.05
    n = len(pts)
    nrm = _table_normals(n)
    assert int(np.sum(~CO.usable(pts, r, nrm))) == 5983
    want = CO.clusters(pts, r, nrm, min_cos, oriented)
    assert want[1] == count and want[2][0] == largest
    assert int(np.sum(want[0] == -1)) == 5983
    t = kdtree.New(pts)
    _check(_raw(t, r, nrm, min_cos, oriented), want, ("grid", min_cos, oriented))
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    _check(_raw(t, r, nrm, min_cos, oriented), want, ("walk", min_cos, oriented))
    monkeypatch.delenv("PCGX_RANGE_WALK")
    if oriented and min_cos == 0.75:  # ... and once on a handle that has seen DeletePoint, curvature on top
        gone = _deleted_ids(n)
        cut = pts.copy()
        cut[gone] = nan
        cur = np.random.default_rng(74).choice(f32([0.0, 0.1, 0.25, 0.5, nan]), n)
        want_d = CO.clusters(cut, r, nrm, min_cos, oriented, cur, 0.25, 2, 40)
        td = kdtree.New(pts)
        td.DeletePoints(gone)
        _check(_raw(td, r, nrm, min_cos, oriented, cur, 0.25, 2, 40), want_d, "deleted")
        _check(_raw(t, r, nrm, min_cos, oriented, cur, 0.25, 2, 40), CO.clusters(pts, r, nrm, min_cos, oriented, cur, 0.25, 2, 40),
               "grid, curvature")


# ------------------------------------------------------------------------------------------------ 4. cube faces

def _faces():
    parts, normals, face = [], [], []
    for axis in range(3):
        uv = np.random.default_rng(80 + axis).random((4000, 2)).astype(f32)
        p = np.zeros((4000, 3), f32)
        p[:, [k for k in range(3) if k != axis]] = uv
        e = np.zeros(3, f32)
        e[axis] = 1.0
        parts.append(p)
        normals.append(np.tile(e, (4000, 1)))
        face.append(np.full(4000, axis))
    perm = np.random.default_rng(90).permutation(12_000)
    return (np.ascontiguousarray(np.concatenate(parts)[perm]), np.ascontiguousarray(np.concatenate(normals)[perm]),
            np.concatenate(face)[perm])


def test_three_faces_of_a_cube():
    pts, nrm, face = _cached("faces", _faces)
    n, r = len(pts), 0.05
    t = kdtree.New(pts)
    want = CO.clusters(pts, r)
    assert want[1] == 1 and want[2][0] == 12_000
    _check(_raw(t, r), want, "euclidean")
    want = CO.clusters(pts, r, nrm, 0.9, False)
    assert want[1] == 3 and want[2][:3].tolist() == [4000] * 3
    firsts = [int(np.nonzero(face == a)[0][0]) for a in range(3)]
    assert [int(want[0][i]) for i in sorted(firsts)] == [0, 1, 2]  # equal sizes: numbered by their smallest ids
    assert all(len(set(want[0][face == a].tolist())) == 1 for a in range(3))
    got = _raw(t, r, nrm, 0.9, False)
    _check(got, want, "analytic normals")
    # the chain a user runs: the library's normals and curvature, the limit at the median curvature
    lib_n, lib_c, _ = t.Normals(r)
    max_c = float(np.nanmedian(lib_c))
    want = CO.clusters(pts, r, lib_n, 0.9, False, lib_c, max_c)
    got = _raw(t, r, lib_n, 0.9, False, lib_c, max_c)
    _check(got, want, "computed normals")
    ce = segmentation.ClusterExtraction(t, ClusterTolerance=r)
    ce.SetInputNormals(lib_n, MinCos=0.9)
    ce.SetInputCurvature(lib_c, max_c)
    parts = ce.Extract()
    assert len(parts) == want[1] and np.array_equal(np.concatenate(parts), want[3][:int(want[2].sum())])
    assert [len(p) for p in parts] == want[2][:want[1]].tolist() and np.array_equal(ce.labels, want[0])
    shares = []
    for a in range(3):  # more than three quarters of each face's interior (> 0.1 from every edge) under one label
        uv = pts[:, [k for k in range(3) if k != a]]
        inner = (face == a) & np.all((uv > 0.1) & (uv < 0.9), axis=1)
        lab = got[0][inner]
        best = np.bincount(lab[lab >= 0]).argmax() if np.any(lab >= 0) else -1
        shares.append((int(best), float(np.mean(lab == best))))
    print("clusters with computed normals:", got[1], "largest:", got[2][:5].tolist(), "interior shares:", shares)
    assert all(s > 0.75 for _, s in shares), shares
    assert len({b for b, _ in shares}) == 3, shares


# ------------------------------------------------------------------------------------------------ 5. coincident heaps

@pytest.mark.parametrize("r", [0.5, 1.5])
def test_coincident_heaps(r, monkeypatch):
    pts = _cached("heaps", lambda: _heap_scene(10_000))
    n = len(pts)
    ref = _components_reference(pts, np.zeros(n, np.uint32), r)  # the smallest id of every point's component
    want = CO.clusters(pts, r)
    heap_ids = [np.nonzero(np.all(pts == h, axis=1))[0] for h, _ in HEAPS]
    assert [len(i) for i in heap_ids] == [4095, 4096, 4097, 6000]
    for name, t, _ in _handles(pts, monkeypatch, rows=False):
        got = _raw(t, r)
        _check(got, want, (name, r))
        labels, c, sizes, _ = got
        assert np.all(labels >= 0)
        low = np.full(c, n, np.int64)
        np.minimum.at(low, labels, np.arange(n))
        assert np.array_equal(low[labels], ref), (name, r)  # the same partition as the union-find over brute-force pairs
        heap_labels = [set(labels[i].tolist()) for i in heap_ids]
        assert all(len(s) == 1 for s in heap_labels)
        if r == 0.5:  # each heap a cluster of exactly its own size
            assert [int(sizes[next(iter(s))]) for s in heap_labels] == [4095, 4096, 4097, 6000], (name, r)
            assert len(set.union(*heap_labels)) == 4
        else:  # the heaps are one cluster
            assert len(set.union(*heap_labels)) == 1


# ------------------------------------------------------------------------------------------------ 6. a long chain

def test_a_long_chain():
    """50 000 points 0.25 apart (exact in float32), ids shuffled; the expected output is written down, no brute force"""
    n = 50_000
    perm = np.random.default_rng(60).permutation(n)  # the k-th point along the line has id perm[k]
    pts = np.zeros((n, 3), f32)
    pts[perm, 0] = f32(0.25) * np.arange(n, dtype=f32)
    assert np.array_equal(np.sort(pts[:, 0]).astype(np.float64), 0.25 * np.arange(n))
    t = kdtree.New(pts)
    print("chain: grid on =", _grid_on(t)[3])  # which source the handle took
    ar = np.arange(n)
    # DistSq == r^2 is not below it: no edge
    _check(_raw(t, 0.25), (ar, n, np.ones(n, np.int64), ar), "r = 0.25")
    up = float(np.nextafter(f32(0.25), f32(1)))
    sizes = np.zeros(n, np.int64)
    sizes[0] = n
    _check(_raw(t, up), (np.zeros(n, np.int64), 1, sizes, ar), "one cluster")
    # without every 1000th point: 50 runs of 999, numbered by their smallest ids
    k = np.arange(n)
    keep = k % 1000 != 0
    m = int(keep.sum())
    perm2 = np.random.default_rng(61).permutation(m)
    pts2 = np.zeros((m, 3), f32)
    pts2[perm2, 0] = f32(0.25) * k[keep].astype(f32)
    run = (k[keep] // 1000)  # the run of the j-th kept point along the line; its id is perm2[j]
    low = np.full(50, m, np.int64)
    np.minimum.at(low, run, perm2)
    number = np.empty(50, np.int64)
    number[np.argsort(low)] = np.arange(50)
    labels = np.empty(m, np.int64)
    labels[perm2] = number[run]
    sizes = np.zeros(m, np.int64)
    sizes[:50] = 999
    t2 = kdtree.New(pts2)
    print("cut chain: grid on =", _grid_on(t2)[3])
    _check(_raw(t2, up), (labels, 50, sizes, np.argsort(labels, kind="stable")), "50 runs")


# ------------------------------------------------------------------------------------------------ 7. edges of the contract

def test_small_and_degenerate_clouds():
    # (Len() == 0 is PCGX_OK by the contract, but no handle can be empty: pcgx_kdtree_build refuses one)
    one = kdtree.New(f32([[1, 2, 3]]))
    _check(_raw(one, 0.1), (np.array([0]), 1, np.array([1]), np.array([0])), "Len() 1")
    _check(_raw(one, 0.1, min_size=2), (np.array([-1]), 0, np.array([0]), np.array([-1])), "Len() 1, too small")
    _check(_raw(one, 0.1, f32([[0, 0, 0]])), (np.array([-1]), 0, np.array([0]), np.array([-1])), "Len() 1, zero normal")
    for n in (2, 63, 64, 65, 257):
        rng = np.random.default_rng(100 + n)
        pts = (rng.integers(0, 6, (n, 3)) / 8.0).astype(f32)
        nrm = TABLE[rng.integers(0, 10, n)]
        t = kdtree.New(pts)
        for r in (0.125, 0.13, 0.3):
            _check(_raw(t, r), CO.clusters(pts, r), (n, r))
            _check(_raw(t, r, nrm, 0.75, True), CO.clusters(pts, r, nrm, 0.75, True), (n, r, "normals"))
    # NaN points only
    n = 100
    t = kdtree.New(np.full((n, 3), nan, f32))
    none = (np.full(n, -1), 0, np.zeros(n, np.int64), np.full(n, -1))
    _check(_raw(t, 0.5), none, "NaN cloud")
    # all normals zero: every label -1 and C = 0; a NaN curvature everywhere does the same
    pts = synth.uniform_cloud(1000, 1.0, 75)
    t = kdtree.New(pts)
    none = (np.full(1000, -1), 0, np.zeros(1000, np.int64), np.full(1000, -1))
    _check(_raw(t, 0.1, np.zeros((1000, 3), f32)), none, "zero normals")
    _check(_raw(t, 0.1, curvature=np.full(1000, nan, f32), max_curvature=inf), none, "NaN curvature")
    # infinite coordinates among finite ones: unusable, and nobody's neighbour (inf - inf is NaN, inf - x is inf)
    pts2 = pts.copy()
    pts2[3::11, 1] = inf
    pts2[5::13, 2] = -inf
    want = CO.clusters(pts2, 0.1)
    assert np.all(want[0][3::11] == -1) and np.all(want[0][5::13] == -1) and want[1] > 1
    _check(_raw(kdtree.New(pts2), 0.1), want, "inf points")
    # NaN coordinates among finite ones: the neighbourhoods are Range's on that handle, whose tree a NaN puts out of
    # order as it does the reference's, so no brute force says what they are -- but a NaN point is never usable
    pts3 = pts.copy()
    pts3[::7] = nan
    labels, c, sizes, ids = _raw(kdtree.New(pts3), 0.1)
    assert np.all(labels[::7] == -1) and np.all(np.delete(labels, np.arange(0, 1000, 7)) >= 0)
    assert np.array_equal(np.bincount(labels[labels >= 0], minlength=1000), sizes) and c == int(np.sum(sizes > 0))
    members = np.nonzero(labels >= 0)[0]
    assert np.array_equal(ids[:len(members)], members[np.argsort(labels[members], kind="stable")])
    assert np.all(ids[len(members):] == -1) and np.all(np.diff(sizes[:c]) <= 0)
    # every point deleted
    td = kdtree.New(pts)
    td.DeletePoints(np.arange(1000))
    _check(_raw(td, 0.1), none, "all deleted")


def test_each_optional_output_left_out():
    pts = synth.uniform_cloud(3000, 1.0, 76)
    t = kdtree.New(pts)
    want = CO.clusters(pts, 0.06, min_size=2)
    for ws, wi in ((False, True), (True, False), (False, False)):
        labels, c, sizes, ids = _call(t, 0.06, None, 0.0, 0, None, 0.0, 2, 0, ws, wi)
        assert c == want[1] and np.array_equal(labels, want[0])
        assert np.array_equal(sizes, want[2]) if ws else np.all(sizes == -7)
        assert np.array_equal(ids, want[3]) if wi else np.all(ids == -7)


def test_bad_arguments():
    lib = L.lib()
    pts = synth.uniform_cloud(100, 1.0, 90)
    t = kdtree.New(pts)
    nrm = np.tile(f32([0, 0, 1]), (100, 1))
    cur = np.zeros(100, f32)
    lab, siz, ids = (np.zeros(100, np.int64) for _ in range(3))
    lab32 = np.zeros(100, np.int32)
    cnt = C.c_int64(5)
    E = L.PCGX_E_INVALID

    def call(h=t._h, r=0.1, n=None, mc=0.0, c=None, xc=0.0, lo=1, hi=0, labels=lab, count=C.byref(cnt)):
        return lib.pcgx_kdtree_clusters(h, r, _opt(n), mc, 0, _opt(c), xc, lo, hi, _opt(labels), count, L.ptr(siz), L.ptr(ids))

    assert call() == L.PCGX_OK
    for r in (0.0, -1.0, inf, nan):
        assert call(r=r) == E
        assert lib.pcgx_kdtree_clusters_dev(t._h, r, None, 0.0, 0, None, 0.0, 1, 0, L.ptr(lab32), L.ptr(lab32), None, None,
                                            None) == E
    assert call(n=nrm, mc=nan) == E and call(mc=nan) == L.PCGX_OK        # a NaN min_cos counts with normals only
    assert call(c=cur, xc=nan) == E and call(xc=nan) == L.PCGX_OK        # ... a NaN max_curvature with curvature only
    assert call(lo=-1) == E and call(hi=-1) == E
    assert call(lo=5, hi=4) == E and call(lo=5, hi=5) == L.PCGX_OK       # 0 < max_size < max(min_size, 1)
    assert call(lo=0, hi=1) == L.PCGX_OK and call(lo=5, hi=0) == L.PCGX_OK
    assert call(h=None) == E
    assert call(labels=None) == E and call(count=None) == E
    assert lib.pcgx_kdtree_clusters_dev(None, 0.1, None, 0.0, 0, None, 0.0, 1, 0, L.ptr(lab32), L.ptr(lab32), None, None,
                                        None) == E
    assert lib.pcgx_kdtree_clusters_dev(t._h, 0.1, None, 0.0, 0, None, 0.0, 1, 0, None, L.ptr(lab32), None, None, None) == E
    assert lib.pcgx_kdtree_clusters_dev(t._h, 0.1, None, 0.0, 0, None, 0.0, 1, 0, L.ptr(lab32), None, None, None, None) == E
    with pytest.raises(ValueError):
        t.Clusters(0.1, Normals=nrm[:50])
    with pytest.raises(ValueError):
        t.Clusters(0.1, Curvature=cur[:50])


# ------------------------------------------------------------------------------------------------ 8. the device form

def test_device_form_on_two_streams():
    """ClustersDev on torch tensors on a non-default stream equals the host form on scenes 1 and 3, a second
    independent call on another stream beside it; nothing but the final copies is read back"""
    import torch
    dev = torch.device("cuda", 0)
    pts = _cloud()
    n = len(pts)
    nrm = _table_normals(n)
    t = kdtree.New(pts)
    other = synth.uniform_cloud(5000, 1.0, 77)
    t2 = kdtree.New(other)
    want1 = CO.rank_and_group(n, _names("cloud", pts, 0.032), 5, 0)
    want3 = CO.clusters(pts, 0.05, nrm, 0.75, False)
    want_o = CO.clusters(other, 0.05)

    def outs(m):
        return [torch.full((k,), -7, dtype=torch.int32, device=dev) for k in (m, 1, m, m)]

    def host(o):
        lab, cnt, siz, ids = (x.cpu().numpy().astype(np.int64) for x in o)
        return lab, int(cnt[0]), siz, ids

    dn = torch.from_numpy(nrm).to(dev)
    o1, o3, oo, o1b = outs(n), outs(n), outs(5000), outs(n)
    s_a, s_b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s_a):
        t.ClustersDev(0.032, o1[0].data_ptr(), o1[1].data_ptr(), o1[2].data_ptr(), o1[3].data_ptr(), MinSize=5,
                      stream=s_a.cuda_stream)
    with torch.cuda.stream(s_b):
        t2.ClustersDev(0.05, oo[0].data_ptr(), oo[1].data_ptr(), oo[2].data_ptr(), oo[3].data_ptr(), stream=s_b.cuda_stream)
    with torch.cuda.stream(s_a):
        t.ClustersDev(0.05, o3[0].data_ptr(), o3[1].data_ptr(), o3[2].data_ptr(), o3[3].data_ptr(), d_normals=dn.data_ptr(),
                      MinCos=0.75, stream=s_a.cuda_stream)
        t.ClustersDev(0.032, o1b[0].data_ptr(), o1b[1].data_ptr(), MinSize=5, stream=s_a.cuda_stream)  # (no optional outputs)
    s_a.synchronize()
    s_b.synchronize()
    torch.cuda.synchronize()
    _check(host(o1), want1, "scene 1, device")
    _check(host(o3), want3, "scene 3, device")
    _check(host(oo), want_o, "other stream")
    lab, cnt, siz, ids = host(o1b)
    assert cnt == want1[1] and np.array_equal(lab, want1[0]) and np.all(siz == -7) and np.all(ids == -7)
    # ... and the host form of the same
    _check(_raw(t, 0.032, min_size=5), want1, "scene 1, host")
    _check(_raw(t, 0.05, nrm, 0.75, False), want3, "scene 3, host")
