"""GPU: farthest-point sampling (csrc/fps.hip, csrc/fps_terms.h, csrc/fps_plan.h; include/pcgx.h, "farthest-point
sampling") against the NumPy oracle (tests/fps_oracle.py), everything by array_equal: a maximum with a fixed tie rule
is a property of the point set, so ids, the bits of dist_sq and cover_sq, owners and the padding tails are the oracle's
on the grid handle, under the forced walk and after DeletePoints, whatever tiles a pick skipped.  Every call is made
twice: the same bits on every call.  (Every pick runs the wide kernel: the one-workgroup form lost its measurement and
went, with its knob -- DESIGN.md 3.28 -- so there is one setting to test.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import kdtree, sampling, synth
from pcgol_amd.pc import PointCloud, PointCloudHeader

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_oracle as FO  # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
nan, inf = np.nan, np.inf


def _plan(n, count):
    out = np.zeros(4, np.int64)
    L.check(L.lib().pcgx_fps_plan(int(n), int(count), L.ptr(out)))
    return dict(tile=int(out[0]), tiles=int(out[1]), wg_tiles=int(out[2]), workgroups=int(out[3]))


def _raw(t, count, start=-1):
    """the host entry point's whole output, into buffers pre-filled with a pattern"""
    n = t.Len()
    ids = np.full(count, -7, np.int64)
    dsq = np.full(count, -7.0, f32)
    cover = np.full(1, -7.0, f32)
    own = np.full(n, -7, np.int64)
    cnt = C.c_int64(-7)
    L.check(L.lib().pcgx_kdtree_fps(t._h, count, start, L.ptr(ids), C.byref(cnt), L.ptr(dsq), L.ptr(cover), L.ptr(own)))
    return ids, cnt.value, dsq, cover[0], own


def _check(t, count, want, start=-1, what=""):
    for _ in range(2):  # the same bits on every call
        ids, m, dsq, cover, own = _raw(t, count, start)
        assert m == want["n_ids"], (what, m, want["n_ids"])
        bad = np.nonzero(ids != want["ids"])[0]
        assert len(bad) == 0, (what, bad[:5], ids[bad[:5]], want["ids"][bad[:5]])
        assert np.array_equal(FO.bits(dsq), FO.bits(want["dist_sq"])), what
        assert FO.bits(cover)[0] == FO.bits(want["cover_sq"])[0], (what, cover, want["cover_sq"])
        assert np.array_equal(own, want["owner"]), (what, np.nonzero(own != want["owner"])[0][:10])
    return ids, m, dsq, cover, own


def _surface(n, seed=33):
    return np.ascontiguousarray(synth.surface_cloud(n, 5.0, seed)[0], f32)


# ------------------------------------------------------------------------------------------------ every kind of handle

def test_every_kind_of_handle(monkeypatch):
    """20 000 surface points, count 300: the grid handle, the forced walk, and a handle that lost 10 % of its points,
    id 0 (the default start) and two of the oracle's early picks among them; Start = -1 and an explicit start"""
    pts = _surface(20_000)
    n = len(pts)
    assert _plan(n, 300)["tiles"] > 2 * _plan(n, 300)["wg_tiles"]
    t = kdtree.New(pts)
    for start in (-1, 4321):
        want = FO.fps(pts, 300, start)
        assert want["n_ids"] == 300 and want["ids"][0] == (0 if start < 0 else start)
        assert np.isinf(want["dist_sq"][0]) and np.all(np.diff(want["dist_sq"][1:]) <= 0) and want["cover_sq"] > 0
        _check(t, 300, want, start, ("grid", start))
        monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        _check(t, 300, want, start, ("walk", start))
        monkeypatch.delenv("PCGX_RANGE_WALK")
    early = FO.fps(pts, 300)["ids"]
    gone = np.unique(np.concatenate([np.random.default_rng(63).choice(n, n // 10, replace=False), [0, early[1], early[5]]]))
    gone = gone[gone != 4321]
    deleted = np.zeros(n, bool)
    deleted[gone] = True
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    for start in (-1, 4321):
        want = FO.fps(pts, 300, start, deleted=deleted)
        ids, m, _, _, own = _check(td, 300, want, start, ("deleted", start))
        assert not np.isin(ids, gone).any() and np.all(own[gone] == -1) and not np.isin(own, gone).any()
    assert FO.fps(pts, 300, deleted=deleted)["ids"][0] == np.flatnonzero(~deleted)[0] != 0


def test_prefix():
    """count 50 is the first 50 of count 500 on the same handle, and its cover_sq is that call's dist_sq[50]"""
    pts = _surface(20_000, 34)
    t = kdtree.New(pts)
    a, b = _raw(t, 50), _raw(t, 500)
    assert a[1] == 50 and b[1] == 500
    assert np.array_equal(a[0], b[0][:50]) and np.array_equal(FO.bits(a[2]), FO.bits(b[2][:50]))
    assert FO.bits(a[3])[0] == FO.bits(b[2][50])[0]
    want = FO.fps(pts, 500)
    assert np.array_equal(b[0], want["ids"]) and np.array_equal(b[4], want["owner"])


# ------------------------------------------------------------------------------------------------ ties

def test_exact_ties_and_equal_bounds():
    """a 17 x 17 x 3 lattice at spacing 2^-7, count = Len(): every distance exact, nearly every pick a tie, many tiles
    at exactly fps_box_lower == the tile's largest d; the order is the oracle's to the last point"""
    g = np.stack(np.meshgrid(np.arange(17), np.arange(17), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    pts = np.ascontiguousarray(g[np.random.default_rng(7).permutation(len(g))] * f32(2.0 ** -7), f32)
    n = len(pts)
    assert n == 867 and _plan(n, n)["tiles"] == 4
    want = FO.fps(pts, n)
    d = want["dist_sq"][1:]
    assert want["n_ids"] == n and (np.diff(d) == 0).sum() > n // 2 and want["cover_sq"] == -1.0
    t = kdtree.New(pts)
    _check(t, n, want, -1, "lattice")
    _check(t, n, FO.fps(pts, n, 500), 500, "lattice from 500")


def test_coincident_heaps():
    """heaps of 4095 / 4096 / 4097 coincident points and 50 scattered ones, count = 50 + 3 + 20: after the spread points
    the heaps' members come in ascending id order at d = 0, none twice"""
    rng = np.random.default_rng(11)
    sizes = (4095, 4096, 4097)
    centres = f32([[0.2, 0.2, 0.2], [0.8, 0.3, 0.5], [0.4, 0.9, 0.7]])
    pts = np.concatenate([np.tile(c, (m, 1)) for c, m in zip(centres, sizes)] + [rng.random((50, 3), dtype=f32)])
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))], f32)
    count = 50 + 3 + 20
    want = FO.fps(pts, count)
    assert want["n_ids"] == count and np.all(want["dist_sq"][53:] == 0) and np.all(want["dist_sq"][1:53] > 0)
    assert np.all(np.diff(want["ids"][53:]) > 0) and len(np.unique(want["ids"])) == count and want["cover_sq"] == 0
    t = kdtree.New(pts)
    ids, _, _, _, own = _check(t, count, want, -1, "heaps")
    # a zero-distance pick is owned by the earlier pick it coincides with, not by itself
    assert np.all(own[ids[53:]] != ids[53:]) and np.all(own[ids[:53]] == ids[:53])


# ------------------------------------------------------------------------------------------------ what is not eligible

def _with_non_finite(seed):
    rng = np.random.default_rng(seed)
    pts = rng.random((300, 3), dtype=f32)
    bad = rng.choice(300, 40, replace=False)
    pts[bad[:15], 0] = inf
    pts[bad[15:30], 2] = -inf
    pts[bad[30:], :] = inf
    return pts, np.sort(bad)


def test_count_beyond_the_eligible_points():
    """300 points, 40 of them with a +-inf or NaN coordinate, count 400: 260 picks, the tails -1 / -1.0f, cover_sq
    -1.0f, owners -1 on the 40"""
    pts, bad = _with_non_finite(21)
    for with_nan in (False, True):
        if with_nan:  # a tree built with a NaN coordinate
            pts = pts.copy()
            pts[bad[::3], 1] = nan
        want = FO.fps(pts, 400)
        assert want["n_ids"] == 260 and np.all(want["ids"][260:] == -1) and np.all(want["dist_sq"][260:] == -1.0)
        assert want["cover_sq"] == -1.0 and np.all(want["owner"][bad] == -1) and not np.isin(bad, want["ids"]).any()
        t = kdtree.New(pts)
        _check(t, 400, want, -1, ("beyond", with_nan))
        first_ok = int(np.flatnonzero(np.isfinite(pts).all(axis=1))[3])
        _check(t, 400, FO.fps(pts, 400, first_ok), first_ok, ("beyond, start", with_nan))
    none = np.full((64, 3), nan, f32)
    none[::2] = inf
    want = FO.fps(none, 5)
    assert want["n_ids"] == 0 and want["cover_sq"] == -1.0
    _check(kdtree.New(none), 5, want, -1, "empty E")


def test_overflow_to_infinity():
    """64 points at coordinates of magnitude 3e19 among 500 ordinary ones: their squares overflow, d = +inf ties go to
    the smallest id"""
    rng = np.random.default_rng(31)
    pts = rng.random((564, 3), dtype=f32)
    far = rng.choice(564, 64, replace=False)
    pts[far] = (rng.choice(f32([-3e19, 3e19]), (64, 3)) * (1 + rng.random((64, 3), dtype=f32) * f32(0.01))).astype(f32)
    want = FO.fps(pts, 200)
    # (the far points sit in the eight octants: a pick in each has d = +inf, the next pick a finite but huge one)
    assert np.isinf(want["dist_sq"][:8]).all() and np.isfinite(want["dist_sq"][12:]).all() and want["n_ids"] == 200
    t = kdtree.New(pts)
    _check(t, 200, want, -1, "overflow")
    _check(t, 564, FO.fps(pts, 564, int(far[0])), int(far[0]), "overflow, far start")


def test_far_off_points():
    """the ordinary cloud translated by 1e6: coordinates a few ulps apart, many exact ties"""
    pts = np.ascontiguousarray(_surface(5000, 35) + f32(1e6), f32)
    want = FO.fps(pts, 300)
    assert want["n_ids"] == 300
    _check(kdtree.New(pts), 300, want, -1, "far off")


# ------------------------------------------------------------------------------------------------ sizes

def _cloud(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=f32)


def test_small_sizes():
    """Len() 1 to 129, count = Len() + 1: every point is picked and the slot after them is padding"""
    for n in range(1, 130):
        pts = _cloud(n, 100 + n)
        want = FO.fps(pts, n + 1)
        assert want["n_ids"] == n
        ids, m, dsq, cover, own = _raw(kdtree.New(pts), n + 1)
        assert m == n and np.array_equal(ids, want["ids"]) and np.array_equal(FO.bits(dsq), FO.bits(want["dist_sq"])), n
        assert cover == -1.0 and np.array_equal(own, want["owner"]), n


def test_sizes_at_the_seams():
    """Len() one less than, equal to and one more than a tile and a pick workgroup's tiles (read from the plan)"""
    p = _plan(100_000, 10)
    tile, group = p["tile"], p["tile"] * p["wg_tiles"]
    assert tile > 1 and group > tile
    for n in (tile - 1, tile, tile + 1, group - 1, group, group + 1, 2 * group + tile + 3):
        pts = _cloud(n, n)
        q = _plan(n, 40)
        assert q["tiles"] == -(-n // tile) and q["workgroups"] == -(-q["tiles"] // q["wg_tiles"])
        for start in (-1, n - 1):
            _check(kdtree.New(pts), 40, FO.fps(pts, 40, start), start, (n, start))


# ------------------------------------------------------------------------------------------------ device form, filters

def _dev(t, count, start=-1, stream=None, dist=True, cover=True, owner=True, bufs=None):
    import torch
    dev = torch.device("cuda", 0)
    n = t.Len()
    if bufs is None:
        bufs = (torch.full((max(count, 1),), -7, dtype=torch.int32, device=dev), torch.full((1,), -7, dtype=torch.int32, device=dev),
                torch.full((max(count, 1),), -7.0, dtype=torch.float32, device=dev), torch.full((1,), -7.0, dtype=torch.float32, device=dev),
                torch.full((n,), -7, dtype=torch.int32, device=dev))
    ids, m, dsq, cov, own = bufs
    t.FarthestPointsDev(count, ids.data_ptr(), m.data_ptr(), dsq.data_ptr() if dist else 0, cov.data_ptr() if cover else 0,
                        own.data_ptr() if owner else 0, Start=start, stream=stream.cuda_stream if stream else 0)
    return bufs


def test_dev_form_gives_the_host_forms_bits():
    import torch
    pts = _surface(20_000, 36)
    t = kdtree.New(pts)
    count = 200
    h_ids, h_m, h_dsq, h_cover, h_own = _raw(t, count, 77)
    want = FO.fps(pts, count, 77)
    assert np.array_equal(h_ids, want["ids"])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        bufs = _dev(t, count, 77, stream)
        _dev(t, count, 77, stream, bufs=bufs)  # twice in a row into the same buffers
        a = _dev(t, count, 77, stream, dist=False)
        b = _dev(t, count, 77, stream, cover=False)
        c = _dev(t, count, 77, stream, owner=False)
        z = _dev(t, 0, -1, stream)
    stream.synchronize()
    for k, got in enumerate((bufs, a, b, c)):
        ids, m, dsq, cov, own = [x.cpu().numpy() for x in got]
        assert m[0] == h_m and np.array_equal(ids, h_ids), k
        assert np.array_equal(FO.bits(dsq), FO.bits(h_dsq)) if k != 1 else np.all(dsq == -7.0), k
        assert FO.bits(cov)[0] == FO.bits(h_cover)[0] if k != 2 else cov[0] == -7.0, k
        assert np.array_equal(own, h_own) if k != 3 else np.all(own == -7), k
    ids, m, dsq, cov, own = [x.cpu().numpy() for x in z]
    assert m[0] == 0 and cov[0] == -1.0 and np.all(own == -1) and ids[0] == -7 and dsq[0] == -7.0  # count 0: no slot
    got = t.FarthestPoints(count, Start=77, Owner=True)
    assert np.array_equal(got[0], h_ids) and np.array_equal(got[3], h_own) and got[2] == h_cover


def test_filters_give_the_records_in_pick_order():
    import torch
    rng = np.random.default_rng(81)
    xyz = np.ascontiguousarray(_surface(5000, 37))
    bad = rng.choice(len(xyz), 50, replace=False)
    xyz[bad[:30]] = nan
    xyz[bad[30:40], 1] = inf
    xyz[bad[40:], 2] = -inf
    n = len(xyz)
    finite = np.nonzero(np.all(np.isfinite(xyz), axis=1))[0]
    assert len(finite) == n - 50
    dev = torch.device("cuda", 0)
    for names, sizes in ((["tag", "x", "y", "z"], 16), (["a", "b", "x", "y", "z", "c", "d", "e"], 32)):
        dt = np.dtype([(k, "<f4" if k in "xyz" else "<u4") for k in names])
        assert dt.itemsize == sizes
        rec = np.zeros(n, dt)
        for k in names:
            rec[k] = xyz[:, "xyz".index(k)] if k in "xyz" else rng.integers(0, 1 << 32, n, dtype=np.uint64)
        data = np.ascontiguousarray(rec.view(np.uint8))
        hdr = PointCloudHeader(names, [4] * len(names), [1] * len(names), ["F" if k in "xyz" else "U" for k in names], Width=n)
        pp = PointCloud(hdr, n, data)
        assert pp.Stride() == sizes and pp.xyz_offset() == 4 * names.index("x")
        for count, start in ((300, -1), (64, 17)):
            picks = finite[FO.fps(xyz[finite], count, start)["ids"]]
            f = sampling.FarthestPoint(count, sampling.WithStart(start))
            out = f.Filter(pp)
            assert out.Points == count and out.PointCloudHeader.Width == count and out.PointCloudHeader.Height == 1
            assert np.array_equal(out.Data.reshape(-1, sizes), data.reshape(n, sizes)[picks])
            assert np.array_equal(f.Filter(pp).Data, out.Data)  # the same bits on every call
            d_in = torch.from_numpy(data.copy()).to(dev)
            d_out = torch.zeros(n * sizes, dtype=torch.uint8, device=dev)
            m = f.FilterDev(d_in.data_ptr(), n, sizes, pp.xyz_offset(), d_out.data_ptr())
            assert m == count and np.array_equal(d_out[: m * sizes].cpu().numpy(), out.Data)
    assert sampling.FarthestPoint(10 ** 6).Filter(pp).Points == len(finite)  # a count beyond the finite records


def test_bad_arguments():
    lib = L.lib()
    pts = _cloud(100, 90)
    pts[5, 1] = inf
    t = kdtree.New(pts)
    t.DeletePoints(np.array([9], np.int64))
    ids = np.full(100, 7, np.int64)
    dsq = np.full(100, 7.0, f32)
    cover = np.full(1, 7.0, f32)
    own = np.full(100, 7, np.int64)
    cnt = C.c_int64(5)
    args = (L.ptr(ids), C.byref(cnt), L.ptr(dsq), L.ptr(cover), L.ptr(own))
    assert lib.pcgx_kdtree_fps(None, 10, -1, *args) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fps(t._h, -1, -1, *args) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fps(t._h, 10, -1, None, C.byref(cnt), L.ptr(dsq), L.ptr(cover), L.ptr(own)) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fps(t._h, 10, -1, L.ptr(ids), None, L.ptr(dsq), L.ptr(cover), L.ptr(own)) == L.PCGX_E_INVALID
    for start in (-2, 100, 5, 9):  # out of range; a non-finite point; a deleted point
        assert lib.pcgx_kdtree_fps(t._h, 10, start, *args) == L.PCGX_E_INVALID, start
        assert lib.pcgx_kdtree_fps_dev(t._h, 10, start, L.ptr(ids), L.ptr(ids), None, None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fps_dev(None, 10, -1, L.ptr(ids), L.ptr(ids), None, None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fps_dev(t._h, -1, -1, L.ptr(ids), L.ptr(ids), None, None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fps_dev(t._h, 10, -1, None, L.ptr(ids), None, None, None, None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_fps_dev(t._h, 10, -1, L.ptr(ids), None, None, None, None, None) == L.PCGX_E_INVALID
    assert cnt.value == 5 and np.all(ids == 7) and np.all(dsq == 7.0) and cover[0] == 7.0 and np.all(own == 7)
    # count 0: no pick, every slot that exists its padding value
    assert lib.pcgx_kdtree_fps(t._h, 0, -1, None, C.byref(cnt), None, L.ptr(cover), L.ptr(own)) == L.PCGX_OK
    assert cnt.value == 0 and cover[0] == -1.0 and np.all(own == -1) and np.all(ids == 7)
    out = np.full(100 * 12, 7, np.uint8)
    m = C.c_int64(-7)
    src = _cloud(100, 91)
    assert lib.pcgx_fps_filter(L.ptr(src), 100, 12, 0, -1, -1, L.ptr(out), C.byref(m)) == L.PCGX_E_INVALID
    assert lib.pcgx_fps_filter(L.ptr(src), 100, 12, 0, 10, -2, L.ptr(out), C.byref(m)) == L.PCGX_E_INVALID
    assert lib.pcgx_fps_filter(L.ptr(src), 100, 12, 0, 10, 100, L.ptr(out), C.byref(m)) == L.PCGX_E_INVALID
    assert lib.pcgx_fps_filter(L.ptr(src), 100, 8, 0, 10, -1, L.ptr(out), C.byref(m)) == L.PCGX_E_BAD_FIELD
    assert lib.pcgx_fps_filter(L.ptr(src), 0, 12, 0, 10, -1, L.ptr(out), C.byref(m)) == L.PCGX_E_NO_POINT
    none = np.full((100, 3), nan, f32)
    assert lib.pcgx_fps_filter(L.ptr(none), 100, 12, 0, 10, -1, L.ptr(out), C.byref(m)) == L.PCGX_E_NO_POINT
    assert lib.pcgx_fps_filter_dev(None, 100, 12, 0, 10, -1, None, C.byref(m), None) == L.PCGX_E_INVALID
    assert m.value == -7 and np.all(out == 7)
    with pytest.raises(L.PcgxError):
        t.FarthestPoints(-1)
