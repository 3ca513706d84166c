"""k nearest neighbours on the GPU (pcgx_kdtree_knearest / _dev, csrc/knearest.hip) against the brute-force oracle
(tests/knn_oracle.py): ids and DistSq bit for bit, counts exact, on every source -- the grid, the forced walk
(PCGX_RANGE_WALK=1), a crowded handle without a grid, the grid's wave-wide fat rows (PCGX_GRID=2) and a handle after
DeletePoints -- and consistent with Range, Nearest, q == NULL and the device entry point."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import kdtree, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_oracle as KO  # noqa: E402

pytestmark = pytest.mark.gpu


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _grid_on(t):
    out = (C.c_int64 * 14)()
    L.check(L.lib().pcgx_debug_grid_stats(t._h, None, 0, 1.0, out))
    return out[3] == 1


def _check(t, pts, q, k, r, exclude=None, what=""):
    ids, dsq, counts = t.KNearestBatch(q, k, r)
    oi, od, oc = KO.knearest(pts, q, k, r, exclude=exclude)
    bad = np.nonzero((ids != oi).any(1) | (dsq.view(np.uint32) != od.view(np.uint32)).any(1) | (counts != oc))[0]
    assert len(bad) == 0, (what, k, r, len(bad), bad[:5], ids[bad[:1]], oi[bad[:1]], dsq[bad[:1]], od[bad[:1]])
    return ids, dsq, counts


def _queries(pts, seed, n):
    lo, hi = pts.min(0), pts.max(0)
    r = _rng(seed)
    inside = (lo + r.random((n, 3)) * (hi - lo)).astype(np.float32)
    outside = (hi + 0.5 + r.random((50, 3))).astype(np.float32)
    bad = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3])
    return np.ascontiguousarray(np.concatenate([inside, pts[:200], outside, bad]), dtype=np.float32)


def _sources(pts, monkeypatch, deleted):
    """(name, tree, excluded ids): the grid, the forced walk, a handle after DeletePoints"""
    t = kdtree.New(pts)
    yield "grid", t, None
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    yield "walk", t, None
    monkeypatch.delenv("PCGX_RANGE_WALK")
    td = kdtree.New(pts)
    td.DeletePoints(deleted)
    yield "deleted", td, deleted


def test_reference_range_table(golden):
    g = golden("ref_kdtree.json")["range"]
    pts = np.float32(g["points"])
    t = kdtree.New(pts)
    for case in g["cases"]:
        q = np.float32([case["p"]])
        for k in (1, 2, 3, 7, 8):
            _check(t, pts, q, k, case["max_range"], what="table")
        # the table's Range answers have no ties: KNearest is their prefix
        want = [n[0] for n in case["neighbors"]]
        got = t.KNearest(case["p"], 3, case["max_range"])
        assert [n.ID for n in got] == want[:3], case


def test_random_cloud_every_source(monkeypatch):
    pts = synth.uniform_cloud(20_000, 1.0, 41)
    q = _queries(pts, 42, 5000)
    deleted = _rng(43).choice(len(pts), 2000, replace=False)
    cases = [(1, 0.05), (2, 0.05), (8, 0.05), (16, 0.05), (64, 0.05), (8, 0.0), (1, np.inf), (16, np.inf),
             (64, np.inf)]
    for name, t, ex in _sources(pts, monkeypatch, deleted):
        if name == "grid":
            assert _grid_on(t)
        for k, r in cases:
            ids, dsq, counts = _check(t, pts, q, k, r, exclude=ex, what=name)
            assert np.all(counts[-4:] == 0) and np.all(ids[-4:] == -1)  # non-finite queries find nothing
        if name != "deleted":
            assert _check(t, pts, q[:50], 64, np.inf, what=name)[2][:50].min() == 64


def test_k_beyond_len(monkeypatch):
    pts = synth.uniform_cloud(40, 1.0, 44)
    q = _queries(pts, 45, 30)
    for name, t, ex in _sources(pts, monkeypatch, np.arange(0, 40, 7)):
        for k in (39, 40, 41, 64):
            ids, dsq, counts = _check(t, pts, q, k, np.inf, exclude=ex, what=name)
        assert counts[0] == 40 - (0 if ex is None else len(ex))


def test_lattice_ties_everywhere(monkeypatch):
    r = _rng(46)
    g = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 0.25
    pts = np.repeat(g, r.integers(1, 5, len(g)), axis=0)
    pts = np.ascontiguousarray(pts[r.permutation(len(pts))], dtype=np.float32)
    q = np.ascontiguousarray(np.concatenate([g[::3], g[::5] + np.float32(0.125), g[::7] + np.float32([0.125, 0, 0])]),
                             dtype=np.float32)
    deleted = r.choice(len(pts), len(pts) // 8, replace=False)
    for name, t, ex in _sources(pts, monkeypatch, deleted):
        for k in (1, 2, 8, 16, 64):
            for rr in (0.3, np.inf):  # 0.3: the boundary falls inside tie runs; DistSq == 0.0625 * n exactly
                _check(t, pts, q, k, rr, exclude=ex, what=name)
        _check(t, pts, q, 7, 0.25, exclude=ex, what=name)  # DistSq == max_range^2 on the lattice: out


def test_fat_rows_and_crowded_handle(monkeypatch):
    """100k coincident points beside a scattered cloud: without PCGX_GRID the heap crowds the grid away (walk);
    PCGX_GRID=2 keeps it, and the heap's rows are scanned by whole waves"""
    h = np.float32([0.5, 0.5, 0.5])
    u = synth.uniform_cloud(20_000, 1.0, 47)
    pts = np.concatenate([u, np.tile(h, (100_000, 1))])
    perm = _rng(48).permutation(len(pts))
    pts = np.ascontiguousarray(pts[perm], dtype=np.float32)
    r = _rng(49)
    near = (h + (r.random((150, 3)) - 0.5) * 0.02).astype(np.float32)
    q = np.ascontiguousarray(np.concatenate([np.tile(h, (100, 1)), near, _queries(u, 50, 1500)]), dtype=np.float32)
    deleted = np.concatenate([np.nonzero(perm >= 20_000)[0][:5000:7], r.choice(len(pts), 500, replace=False)])
    deleted = np.unique(deleted)
    t = kdtree.New(pts)
    assert not _grid_on(t)
    for k in (16, 64):
        _check(t, pts, q, k, np.inf, what="crowded")
        _check(t, pts, q, k, 0.02, what="crowded")
    monkeypatch.setenv("PCGX_GRID", "2")
    for name, t, ex in _sources(pts, monkeypatch, deleted):
        if name == "grid":
            assert _grid_on(t)
        for k in (1, 16, 64):
            _check(t, pts, q, k, np.inf, exclude=ex, what="fat " + name)
        _check(t, pts, q, 16, 0.02, exclude=ex, what="fat " + name)


def test_range_prefix_and_nearest_consistency():
    pts = synth.uniform_cloud(20_000, 1.0, 51)
    q = _queries(pts, 52, 3000)[:-4]
    t = kdtree.New(pts)
    r = 0.08
    offs, rids, rdsq = t.RangeBatch(q, r)
    for k in (1, 8, 16):
        ids, dsq, counts = t.KNearestBatch(q, k, r)
        checked = 0
        for j in range(len(q)):
            a, b = offs[j], offs[j + 1]
            head = rdsq[a:min(b, a + k + 1)]
            if len(head) > 1 and np.any(head[1:] == head[:-1]):
                continue  # a tie in Range's first k+1: Range orders it by walk discovery
            c = min(k, b - a)
            assert counts[j] == c
            assert np.array_equal(ids[j, :c], rids[a:a + c]) and np.array_equal(dsq[j, :c], rdsq[a:a + c]), j
            checked += 1
        assert checked > len(q) * 0.9
    # k = 1 is Nearest wherever the nearest is not tied and lies below max_range^2
    ni, nd = t.NearestBatch(q, r)
    ids, dsq, counts = t.KNearestBatch(q, 2, r)
    untied = (counts == 0) | (counts == 1) | (dsq[:, 1] != dsq[:, 0])
    below = nd < np.float32(r) * np.float32(r)
    sel = untied & below
    assert sel.sum() > len(q) * 0.9
    assert np.array_equal(ids[sel, 0], ni[sel]) and np.array_equal(dsq[sel, 0], nd[sel])
    assert np.all(counts[~below] == 0)


def test_own_points_and_device_entry(monkeypatch):
    import torch
    pts = synth.uniform_cloud(30_000, 1.0, 53)
    deleted = _rng(54).choice(len(pts), 3000, replace=False)
    for name, t, ex in _sources(pts, monkeypatch, deleted):
        a = t.KNearestBatch(None, 16, 0.1)
        b = t.KNearestBatch(pts, 16, 0.1)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), name
        if ex is None:
            assert np.all(a[0][:, 0] == np.arange(len(pts))) and np.all(a[1][:, 0] == 0)  # itself at 0 (no twins)
        else:
            assert not np.isin(a[0], ex).any()
        dev = torch.device("cuda", 0)
        for own in (True, False):
            q = torch.from_numpy(pts).to(dev)
            di = torch.empty((len(pts), 16), dtype=torch.int32, device=dev)
            dd = torch.empty((len(pts), 16), dtype=torch.float32, device=dev)
            dc = torch.empty(len(pts), dtype=torch.int32, device=dev)
            t.KNearestDev(16, 0.1, di.data_ptr(), dd.data_ptr(), dc.data_ptr(),
                          d_q=0 if own else q.data_ptr(), nq=None if own else len(pts))
            torch.cuda.synchronize()
            assert np.array_equal(di.cpu().numpy().astype(np.int64), a[0]), name
            assert np.array_equal(dd.cpu().numpy().view(np.uint32), a[1].view(np.uint32)), name
            assert np.array_equal(dc.cpu().numpy(), a[2]), name
    # a batch that takes the Morton order agrees with one that does not
    t = kdtree.New(pts)
    q = _queries(pts, 55, 20_000)
    big = t.KNearestBatch(q, 8, 0.1)
    for a0 in (0, 7000, 14000):
        small = t.KNearestBatch(q[a0:a0 + 5000], 8, 0.1)
        for x, y in zip(big, small):
            assert np.array_equal(x[a0:a0 + 5000], y)


def test_surface_1m_own_points_equal_range_fill():
    """1M surface points, q == NULL, k = 16: the library's own Range lists, re-sorted by (DistSq, id) and truncated"""
    pts = synth.surface_cloud(1_000_000, 30.0, 6)[0]
    t = kdtree.New(pts)
    assert _grid_on(t)
    k, r = 16, 0.1
    ids, dsq, counts = t.KNearestBatch(None, k, np.inf)
    offs, rids, rdsq = t.RangeBatch(pts, r)
    n = len(pts)
    rc = np.diff(offs)
    qi = np.repeat(np.arange(n), rc)
    order = np.lexsort((rids, rdsq, qi))
    rids, rdsq = rids[order], rdsq[order]
    pos = np.arange(len(rids)) - offs[qi]
    keep = pos < k
    want_i = np.full((n, k), -1, np.int64)
    want_d = np.zeros((n, k), np.float32)
    want_i[qi[keep], pos[keep]] = rids[keep]
    want_d[qi[keep], pos[keep]] = rdsq[keep]
    full = rc >= k
    assert full.mean() > 0.9
    assert np.all(counts == k)
    assert np.array_equal(ids[full], want_i[full]) and np.array_equal(dsq[full].view(np.uint32), want_d[full].view(np.uint32))
    # fewer than k within r: those come first, the rest lie at r or beyond
    part = np.nonzero(~full)[0]
    for j in part[:2000]:
        c = rc[j]
        assert np.array_equal(ids[j, :c], want_i[j, :c]) and np.all(dsq[j, c:] >= np.float32(r) * np.float32(r))


def test_invalid_arguments():
    pts = synth.uniform_cloud(100, 1.0, 56)
    t = kdtree.New(pts)
    ids = np.empty(64 * 100, np.int64)
    dsq = np.empty(64 * 100, np.float32)
    lib = L.lib()
    for k, r in ((0, 1.0), (65, 1.0), (4, float("nan")), (4, -1.0)):
        assert lib.pcgx_kdtree_knearest(t._h, L.ptr(pts), 100, k, r, L.ptr(ids), L.ptr(dsq), None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_knearest(t._h, None, 99, 4, 1.0, L.ptr(ids), L.ptr(dsq), None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_knearest(t._h, L.ptr(pts), 100, 4, np.inf, L.ptr(ids), L.ptr(dsq), None) == 0
    assert lib.pcgx_kdtree_knearest(t._h, L.ptr(pts), 0, 4, 1.0, None, None, None) == 0
