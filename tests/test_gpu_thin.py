"""GPU: minimum-distance subsampling (csrc/thin.hip, csrc/thin_terms.h; include/pcgx.h, "minimum-distance subsampling")
against the NumPy oracle (tests/thin_oracle.py), everything by array_equal: the kept set is the lexicographically first
maximal independent set of the radius graph, a property of the point set, so ids, owners and the -1 tail are the
oracle's on the grid, on the forced walk and after DeletePoints, and the states after R rounds are its too.  Every call
is made twice: the same bits on every call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import kdtree, sampling, synth
from pcgol_amd.pc import PointCloud, PointCloudHeader

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thin_oracle as TO  # noqa: E402
from test_gpu_keypoints import _cached, _compact_tile, _heap_cloud, _heap_ids, _scores  # noqa: E402
from test_gpu_radius_edges import HEAPS, _assert_heap_grid, _grid_on  # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
nan, inf = np.nan, np.inf


def _raw(t, r, seed=0, score=None, owner=True):
    """the host entry point's whole output: (ids [Len()], n_ids, owner [Len()])"""
    n = t.Len()
    score = None if score is None else np.ascontiguousarray(score, f32)
    ids = np.full(n, -7, np.int64)
    own = np.full(n, -7, np.int64) if owner else None
    cnt = C.c_int64(-7)
    L.check(L.lib().pcgx_kdtree_thin(t._h, float(r), int(seed), L.ptr(score), L.ptr(ids), C.byref(cnt), L.ptr(own)))
    return ids, cnt.value, own


def _thin(t, r, seed=0, score=None, what=""):
    """Thin with owners, the output convention checked (ascending ids, then -1 in every remaining slot) -> (ids, owner)"""
    ids, m, own = _raw(t, r, seed, score)
    assert 0 <= m <= len(ids) and np.all(ids[m:] == -1) and np.all(np.diff(ids[:m]) > 0) and np.all(ids[:m] >= 0), what
    again, m2, own2 = _raw(t, r, seed, score)
    assert m2 == m and np.array_equal(ids, again) and np.array_equal(own, own2), what  # the same bits on every call
    return ids[:m], own


def _check(t, r, want, seed=0, score=None, what=""):
    ids, own = _thin(t, r, seed, score, what)
    assert np.array_equal(ids, want[0]), (what, len(ids), len(want[0]), np.setxor1d(ids, want[0])[:10])
    assert np.array_equal(own, want[1]), (what, np.nonzero(own != want[1])[0][:10])
    return ids, own


MODES = [("hash 0", 0, False), ("hash 77", 77, False), ("score", 0, True)]


# ------------------------------------------------------------------------------------------------ every source

def test_thin_on_every_source(monkeypatch):
    """20 000 uniform points, r = 0.08, on the grid, the forced walk and a handle with 10 % of its points deleted"""
    pts = synth.uniform_cloud(20_000, 1.0, 61)
    n, r = len(pts), 0.08
    lists = TO.site_lists(pts, r)
    gone = np.random.default_rng(63).choice(n, n // 10, replace=False)
    lists_d = lists.without(gone)
    t = kdtree.New(pts)
    assert _grid_on(t)[3] == 1
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    kept = {}
    for name, seed, scored in MODES:
        s = _scores(n, 62) if scored else None
        want = TO.thin(pts, r, seed, s, lists=lists)[:2]
        assert 500 < len(want[0]) < 3000, len(want[0])
        _check(t, r, want, seed, s, (name, "grid"))
        monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        _check(t, r, want, seed, s, (name, "walk"))
        monkeypatch.delenv("PCGX_RANGE_WALK")
        wd = TO.thin(pts, r, seed, s, deleted=gone, lists=lists_d)[:2]
        got, own = _check(td, r, wd, seed, s, (name, "deleted"))
        assert not np.isin(got, gone).any() and not np.isin(own, gone).any() and np.all(own[gone] == -1)
        assert len(np.setxor1d(got, want[0])) > 0  # (a deleted kept point frees its neighbours)
        if scored:
            assert np.all(want[1][np.isnan(s)] == -1) and not np.isnan(s[want[0]]).any() and np.isinf(s[want[0]]).any()
        kept[name] = want[0]
    assert len(np.setxor1d(kept["hash 0"], kept["hash 77"])) > 0  # the seed matters


def test_thin_without_a_grid():
    """a heap of coincident points crowds the grid away: the handle walks its tree"""
    u = synth.uniform_cloud(5000, 1.0, 64)
    pts = np.concatenate([u, np.tile(f32([0.5, 0.5, 0.5]), (2000, 1))])
    pts = np.ascontiguousarray(pts[np.random.default_rng(65).permutation(len(pts))], f32)
    t = kdtree.New(pts)
    assert _grid_on(t)[3] == 0
    s = _scores(len(pts), 66)
    for r in (0.08, 0.02):
        lists = TO.site_lists(pts, r)
        for seed, score in ((5, None), (0, s)):
            want = TO.thin(pts, r, seed, score, lists=lists)[:2]
            _check(t, r, want, seed, score, (r, seed))
            assert len(want[0]) > 300


# ------------------------------------------------------------------------------------------------ fat rows

@pytest.mark.parametrize("r", [1.0, 0.75])
def test_fat_rows(r, monkeypatch):
    """heaps of 4095, 4096, 4097 and 6000 coincident points: fat grid rows scanned by whole waves beside a lane's own
    row, on the grid (PCGX_GRID=2), the walk and after DeletePoints; the last wave is a partial one.  Hash mode over the
    whole cloud; score mode with the slab below the heaps out of it (NaN) and the four points at exactly DistSq == 1.0 /
    0.5625 from a heap scored highest."""
    pts = _cached("heap cloud", _heap_cloud)
    n = len(pts)
    assert n % 64 != 0
    heaps = _heap_ids(pts)
    assert [len(h) for h in heaps] == [m for _, m in HEAPS]
    up = pts[:, 2] > 5.0  # the heaps and the sparse points round them
    edge = np.where(up, f32(2.0), f32(nan))  # every heap point 3, the sparse points round them 2, the extra four 5
    for h in heaps:
        edge[h] = 3.0
    edge[n - 4:] = 5.0
    gone = np.concatenate([np.random.default_rng(9).choice(n - 4, n // 50, replace=False), [h[0] for h in heaps[:2]]])
    gone = np.unique(gone)
    lists = _cached(("thin heap lists", r), lambda: TO.site_lists(pts, r))
    monkeypatch.setenv("PCGX_GRID", "2")
    t = kdtree.New(pts)
    _assert_heap_grid(t)
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    # hash mode: every heap keeps exactly one point, its member that comes first
    seed = 3
    want = TO.thin(pts, r, seed, lists=lists)[:2]
    for h in heaps:
        first = int(h[np.argmin(TO.hash_key(seed, h))])
        assert np.intersect1d(want[0], h).tolist() == [first] and np.all(want[1][h] == first)
    _check(t, r, want, seed, None, ("hash", "grid"))
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    _check(t, r, want, seed, None, ("hash", "walk"))
    monkeypatch.delenv("PCGX_RANGE_WALK")
    # score mode (the slab takes no part, so the lists without it serve)
    slab = np.nonzero(~up)[0]
    for name, tree, deleted in (("grid", t, None), ("walk", t, None), ("deleted", td, gone)):
        out = slab if deleted is None else np.union1d(slab, deleted)
        want = TO.thin(pts, r, 0, edge, deleted=out, lists=lists.without(out))[:2]
        if name == "walk":
            monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        ids, own = _check(tree, r, want, 0, edge, ("edge", name))
        monkeypatch.delenv("PCGX_RANGE_WALK", raising=False)
        # a point at exactly DistSq == r^2 does not drop its heap; one strictly inside does, and owns it
        assert set(range(n - 4, n)) <= set(ids.tolist())
        left = [np.setdiff1d(h, gone) if deleted is not None else h for h in heaps]
        first = [[int(h[0])] for h in left]
        assert [np.intersect1d(ids, h).tolist() for h in left] == (first[:2] + [[], []] if r == 1.0 else first)
        owners = [np.unique(own[h]).tolist() for h in left]
        assert owners == (first[:2] + [[n - 2], [n - 1]] if r == 1.0 else first)
        assert np.all(own[slab] == -1) and (deleted is None or np.all(own[deleted] == -1))


# ------------------------------------------------------------------------------------------------ exact spacing, rounds

def _dev(t, r, seed=0, score=None, max_rounds=0, owner=True, stream=None, left=True):
    """ThinDev -> (ids [n] int32, n_ids, owner [n] or None, n_left or None)"""
    import torch
    dev = torch.device("cuda", 0)
    n = t.Len()
    di = torch.full((n,), -7, dtype=torch.int32, device=dev)
    do = torch.full((n,), -7, dtype=torch.int32, device=dev)
    dc = torch.full((2,), -7, dtype=torch.int32, device=dev)
    ds = None if score is None else torch.from_numpy(np.ascontiguousarray(score, f32)).to(dev)
    torch.cuda.synchronize()
    t.ThinDev(r, di.data_ptr(), dc.data_ptr(), dc.data_ptr() + 4 if left else 0, d_owner=do.data_ptr() if owner else 0,
              d_score=ds.data_ptr() if ds is not None else 0, Seed=seed, MaxRounds=max_rounds,
              stream=stream.cuda_stream if stream is not None else 0)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    c = dc.cpu().numpy()
    return di.cpu().numpy(), int(c[0]), do.cpu().numpy() if owner else None, int(c[1]) if left else None


def test_exact_spacing_and_long_chains():
    """600 points on a line at spacing 2^-7, ids permuted, score = -x: a chain of hundreds of rounds"""
    default = L.lib().pcgx_thin_default_rounds()
    pos = np.random.default_rng(3).permutation(600)
    pts = np.zeros((600, 3), f32)
    pts[:, 0] = pos.astype(f32) * f32(2.0 ** -7)
    score = -pts[:, 0]
    t = kdtree.New(pts)
    for r, step in ((f32(4 * 2.0 ** -7), 4), (np.nextafter(f32(4 * 2.0 ** -7), f32(1)), 5)):
        lists = TO.brute_lists(pts, r)
        want = TO.thin(pts, r, 0, score, lists=lists)[:2]
        assert np.array_equal(np.sort(pos[want[0]]), np.arange(0, 600, step))  # distance exactly r is no neighbour
        e = TO.eligible(lists, score)
        states, history = TO.rounds(lists, TO.rank_of(TO.priority_order(e, 0, score), 600))
        assert len(history) > 3 * default  # the host form needs several batches
        _check(t, r, want, 0, score, r)
        for R in (1, 2, 7):
            ids, m, own, left = _dev(t, r, 0, score, max_rounds=R)
            kept = np.nonzero(states[R - 1] == TO.KEPT)[0]
            assert left == history[R - 1] and left > 0
            assert m == len(kept) and np.array_equal(ids[:m], kept) and np.all(ids[m:] == -1)
            assert np.all(own == -2)
        ids, m, own, left = _dev(t, r, 0, score, max_rounds=len(history) + 5)
        assert left == 0 and np.array_equal(ids[:m], want[0]) and np.all(ids[m:] == -1) and np.array_equal(own, want[1])
        assert _dev(t, r, 0, score, max_rounds=len(history) - 1)[3] > 0  # one round short: not yet


# ------------------------------------------------------------------------------------------------ small and edge sizes

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_small_lengths(n):
    rng = np.random.default_rng(80 + n)
    pts = (rng.integers(0, 8, (n, 3)) / 8.0).astype(f32)
    s = _scores(n, 81)
    t = kdtree.New(pts)
    for r in (0.25, 0.13, 5.0):
        lists = TO.brute_lists(pts, r)
        for seed, score in ((0, None), (9, None), (0, s)):
            _check(t, r, TO.thin(pts, r, seed, score, lists=lists)[:2], seed, score, (n, r, seed))


def test_compaction_tile_boundaries_and_nothing_kept():
    tile = _compact_tile()
    for n in (tile - 1, tile, tile + 1, 3 * tile + 5):
        pts = np.ascontiguousarray(np.stack([np.arange(n), np.zeros(n), np.zeros(n)], axis=1), f32)
        pts = pts[np.random.default_rng(n).permutation(n)]
        t = kdtree.New(pts)
        for score in (None, np.ones(n, f32)):  # every point alone in its neighbourhood: everything is kept
            ids, m, own = _raw(t, 0.5, 1, score)
            assert m == n and np.array_equal(ids, np.arange(n)) and np.array_equal(own, np.arange(n))
        ids, m, own = _raw(t, 0.5, 0, np.full(n, nan, f32))
        assert m == 0 and np.all(ids == -1) and np.all(own == -1)
        ids, m, own, left = _dev(t, 0.5, 0, np.full(n, nan, f32))
        assert m == 0 and np.all(ids == -1) and np.all(own == -1) and left == 0
        s = np.ones(n, f32)
        s[::3] = nan
        ids, own = _thin(t, 0.5, 0, s)
        assert np.array_equal(ids, np.nonzero(~np.isnan(s))[0]) and np.array_equal(own, np.where(np.isnan(s), -1, np.arange(n)))


def test_non_finite_coordinates_among_finite_points():
    base = synth.uniform_cloud(3000, 1.0, 91)
    # infinite coordinates among finite ones: outside E, and nobody's neighbour
    pts = base.copy()
    pts[1200] = [0.5, inf, 0.5]
    pts[2999] = [0.5, 0.5, -inf]
    pts[5::13, 2] = inf
    out = np.nonzero(~np.isfinite(pts).all(axis=1))[0]
    t = kdtree.New(pts)
    for seed, score in ((0, None), (0, _scores(len(pts), 92))):
        ids, own = _check(t, 0.1, TO.thin(pts, 0.1, seed, score)[:2], seed, score, "inf")
        assert np.all(own[out] == -1) and not np.isin(out, ids).any()
    # a NaN coordinate as well: the neighbourhoods are Range's on that handle, whose tree a NaN puts out of order, so
    # no brute force says what they are -- the handle's own Range lists do, and the oracle's rule over them is the answer
    pts[17] = [nan, 0.5, 0.5]
    pts[::7, 1] = nan
    out = np.nonzero(~np.isfinite(pts).all(axis=1))[0]
    t = kdtree.New(pts)
    offs, nb, _ = t.RangeBatch(pts, 0.1)
    lists = TO.Lists(offs, nb)
    assert not TO.eligible(lists)[out].any()
    for seed, score in ((0, None), (0, _scores(len(pts), 92))):
        ids, own = _check(t, 0.1, TO.thin(pts, 0.1, seed, score, lists=lists)[:2], seed, score, "nan")
        assert np.all(own[out] == -1) and not np.isin(out, ids).any() and len(ids) > 200


# ------------------------------------------------------------------------------------------------ device forms, filters

def test_dev_form_gives_the_host_forms_bits():
    import torch
    pts = synth.surface_cloud(20_000, 5.0, 33)[0]
    t = kdtree.New(pts)
    s = _scores(len(pts), 34)
    stream = torch.cuda.Stream()
    for seed, score in ((7, None), (0, s)):
        want_ids, want_own = t.Thin(0.1, Seed=seed, Score=score, Owner=True)
        assert len(want_ids) > 200
        with torch.cuda.stream(stream):
            ids, m, own, left = _dev(t, 0.1, seed, score, max_rounds=200 if score is not None else 0, stream=stream)
            assert left == 0 and m == len(want_ids) and np.array_equal(ids[:m], want_ids) and np.all(ids[m:] == -1)
            assert np.array_equal(own, want_own)
            # two calls in a row on that stream; the optional outputs left out one by one
            a = _dev(t, 0.1, seed, score, max_rounds=200 if score is not None else 0, stream=stream, owner=False)
            b = _dev(t, 0.1, seed, score, max_rounds=200 if score is not None else 0, stream=stream, left=False)
        assert a[1] == m and np.array_equal(a[0], ids) and a[3] == 0
        assert b[1] == m and np.array_equal(b[0], ids) and np.array_equal(b[2], own)
    assert np.array_equal(t.Thin(0.1, Seed=7), t.Thin(0.1, Seed=7, Owner=True)[0])


def test_filters_keep_the_records_byte_for_byte():
    import torch
    rng = np.random.default_rng(81)
    xyz = synth.uniform_cloud(20_000, 1.0, 61).copy()
    bad = rng.choice(len(xyz), 50, replace=False)
    xyz[bad[:30]] = nan
    xyz[bad[30:40], 1] = inf
    xyz[bad[40:], 2] = nan
    n = len(xyz)
    dt = np.dtype([("tag", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
    rec = np.zeros(n, dt)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rec["tag"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    data = np.ascontiguousarray(rec.view(np.uint8))
    pp = PointCloud(PointCloudHeader(["tag", "x", "y", "z"], [4, 4, 4, 4], [1, 1, 1, 1], ["U", "F", "F", "F"], Width=n), n, data)
    assert pp.Stride() == 16 and pp.xyz_offset() == 4
    finite = np.nonzero(np.all(np.isfinite(xyz), axis=1))[0]
    f = sampling.MinDistance(0.08, sampling.WithSeed(11))
    kept = finite[kdtree.New(np.ascontiguousarray(xyz[finite])).Thin(0.08, Seed=11)]
    assert np.array_equal(kept, finite[TO.thin(xyz[finite], 0.08, 11)[0]]) and 500 < len(kept) < 3000
    out = f.Filter(pp)
    assert out.Points == len(kept) and out.PointCloudHeader.Width == out.Points and out.PointCloudHeader.Height == 1
    assert np.array_equal(out.Data.reshape(-1, 16), data.reshape(n, 16)[kept])
    assert np.array_equal(f.Filter(pp).Data, out.Data)  # the same bits on every call
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(data.copy()).to(dev)
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    m = f.FilterDev(d_in.data_ptr(), n, 16, 4, d_out.data_ptr())
    assert m == out.Points and np.array_equal(d_out[: m * 16].cpu().numpy(), out.Data)
    assert len(sampling.New(0.08).Filter(pp).Data) != 0 and not np.array_equal(sampling.New(0.08).Filter(pp).Data, out.Data)


def test_bad_arguments():
    lib = L.lib()
    pts = synth.uniform_cloud(100, 1.0, 90)
    t = kdtree.New(pts)
    ids = np.full(100, 7, np.int64)
    own = np.full(100, 7, np.int64)
    cnt = C.c_int64(5)
    for r in (0.0, -1.0, inf, nan, 1e-30, 1e30):  # (the last two: the float32 square is 0 / +inf)
        assert lib.pcgx_kdtree_thin(t._h, r, 0, None, L.ptr(ids), C.byref(cnt), L.ptr(own)) == L.PCGX_E_INVALID
        assert lib.pcgx_kdtree_thin_dev(t._h, r, 0, None, 0, L.ptr(ids), L.ptr(ids), None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_thin(None, 0.1, 0, None, L.ptr(ids), C.byref(cnt), None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_thin(t._h, 0.1, 0, None, None, C.byref(cnt), None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_thin(t._h, 0.1, 0, None, L.ptr(ids), None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_thin_dev(t._h, 0.1, 0, None, -1, L.ptr(ids), L.ptr(ids), None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_thin_dev(t._h, 0.1, 0, None, 0, None, L.ptr(ids), None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_thin_dev(t._h, 0.1, 0, None, 0, L.ptr(ids), None, None, None, None) == L.PCGX_E_INVALID
    assert cnt.value == 5 and np.all(ids == 7) and np.all(own == 7)  # nothing was written
    out = np.full(100 * 12, 7, np.uint8)
    m = C.c_int64(-7)
    for r in (0.0, -1.0, inf, nan):
        assert lib.pcgx_thin_filter(L.ptr(pts), 100, 12, 0, r, 0, L.ptr(out), C.byref(m)) == L.PCGX_E_INVALID
    assert lib.pcgx_thin_filter(L.ptr(pts), 100, 8, 0, 0.1, 0, L.ptr(out), C.byref(m)) == L.PCGX_E_BAD_FIELD
    assert lib.pcgx_thin_filter(L.ptr(pts), 0, 12, 0, 0.1, 0, L.ptr(out), C.byref(m)) == L.PCGX_E_NO_POINT
    none = np.full((100, 3), nan, f32)
    assert lib.pcgx_thin_filter(L.ptr(none), 100, 12, 0, 0.1, 0, L.ptr(out), C.byref(m)) == L.PCGX_E_NO_POINT
    assert lib.pcgx_thin_filter_dev(None, 100, 12, 0, 0.1, 0, None, C.byref(m), None) == L.PCGX_E_INVALID
    assert m.value == -7 and np.all(out == 7)
    with pytest.raises(ValueError):
        t.Thin(0.1, Score=np.ones(99, f32))
