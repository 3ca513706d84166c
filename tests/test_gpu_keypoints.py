"""GPU: local maxima of a per-point score over radius neighbourhoods and ISS keypoints (csrc/keypoints.hip,
csrc/normals.hip's eigenvalue outputs) against tests/keypoints_oracle.py.  Every decision after the eigenvalues is
compared exactly; the eigenvalues themselves within float32 rounding plus the moments' bound of pcgx_kdtree_normals'
contract."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import alignment, features, kdtree, mat, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoints_oracle as KO  # noqa: E402
import pose_oracle as PO  # noqa: E402
from test_gpu_radius_edges import HEAPS, _assert_heap_grid, _grid_on, _heap_scene  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64, u32 = np.float32, np.float64, np.uint32
nan, inf = np.nan, np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _compact_tile():
    """elements per tile of the order-preserving compaction (csrc/bucket_grid.h)"""
    with open(os.path.join(ROOT, "pcgol_amd", "csrc", "bucket_grid.h")) as f:
        return int(re.search(r"constexpr int kRunTile = (\d+);", f.read()).group(1))


def _raw(t, r, score):
    """the host entry point's whole output: (ids [Len()], n_ids)"""
    n = t.Len()
    score = np.ascontiguousarray(score, f32)
    ids = np.full(n, -7, np.int64)
    cnt = C.c_int64(-7)
    L.check(L.lib().pcgx_kdtree_local_maxima(t._h, float(r), L.ptr(score), L.ptr(ids), C.byref(cnt)))
    return ids, cnt.value


def _maxima(t, r, score, what=""):
    """LocalMaxima, with the output convention checked: ascending ids, then -1 in every remaining slot"""
    ids, m = _raw(t, r, score)
    assert 0 <= m <= len(ids) and np.all(ids[m:] == -1) and np.all(np.diff(ids[:m]) > 0) and np.all(ids[:m] >= 0), what
    again, m2 = _raw(t, r, score)
    assert m2 == m and np.array_equal(ids, again), what  # the same bits on every call
    return ids[:m]


def _scores(n, seed):
    """random integers 0..7 (heavy ties), 1 % NaN, 1 % -1, 1 % 0, a few +inf"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 8, n).astype(f32)
    k = max(n // 100, 1)
    pick = rng.permutation(n)
    s[pick[:k]] = nan
    s[pick[k:2 * k]] = -1.0
    s[pick[2 * k:3 * k]] = 0.0
    s[pick[3 * k:3 * k + 5]] = inf
    return s


# ------------------------------------------------------------------------------------------------ LocalMaxima

def test_local_maxima_on_every_source(monkeypatch):
    """20 000 uniform points, r = 0.08, on the grid, the forced walk and a handle with 10 % of its points deleted"""
    pts = synth.uniform_cloud(20_000, 1.0, 61)
    r = 0.08
    s = _scores(len(pts), 62)
    offs, ids = _cached("uniform lists", lambda: KO.brute_lists(pts, r))
    want = KO.maxima_from_lists(s, offs, ids)
    assert 200 < len(want) < 5000 and np.isinf(s[want]).sum() >= 1
    t = kdtree.New(pts)
    assert _grid_on(t)[3] == 1
    assert np.array_equal(_maxima(t, r, s, "grid"), want)
    monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    assert np.array_equal(_maxima(t, r, s, "walk"), want)
    monkeypatch.delenv("PCGX_RANGE_WALK")
    gone = np.random.default_rng(63).choice(len(pts), len(pts) // 10, replace=False)
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    got = _maxima(td, r, s, "deleted")
    assert np.array_equal(got, KO.maxima_from_lists(s, offs, ids, deleted=gone))
    assert not np.isin(got, gone).any() and len(np.setdiff1d(got, want)) > 0  # (a deleted winner frees its neighbours)


def test_local_maxima_without_a_grid():
    """a heap of coincident points crowds the grid away: the handle walks its tree"""
    u = synth.uniform_cloud(5000, 1.0, 64)
    pts = np.concatenate([u, np.tile(f32([0.5, 0.5, 0.5]), (2000, 1))])
    pts = np.ascontiguousarray(pts[np.random.default_rng(65).permutation(len(pts))], f32)
    t = kdtree.New(pts)
    assert _grid_on(t)[3] == 0
    s = _scores(len(pts), 66)
    for r in (0.08, 0.02):
        want = KO.maxima_from_sites(s, KO.sites(pts, r, only=KO.candidate(s)))
        assert np.array_equal(_maxima(t, r, s, r), want) and len(want) > 50


def _heap_ids(pts):
    return [np.nonzero(np.all(pts == h, axis=1))[0] for h, _ in HEAPS]


def _heap_cloud():
    """test_gpu_radius_edges' heap scene, and behind it four points in the heaps' own grid rows: at exactly DistSq == 1.0
    from the first and the second heap, at exactly 0.5625 (= 0.75^2) from the third and the fourth.  (The fourth's also
    lies at exactly 1.0 from the third heap.)"""
    extra = [h + f32([1.0, 0, 0]) for h, _ in HEAPS[:2]] + [h - f32([0.75, 0, 0]) for h, _ in HEAPS[2:]]
    return np.ascontiguousarray(np.concatenate([_heap_scene(), np.array(extra, f32)]), f32)


@pytest.mark.parametrize("r", [1.0, 0.75])
def test_fat_rows(r, monkeypatch):
    """heaps of 4095, 4096, 4097 and 6000 coincident points: fat grid rows scanned by whole waves beside a lane's own
    row, on the grid (PCGX_GRID=2), the walk and after DeletePoints.  The slab below the heaps scores 0 (it is the 20 000
    point test's ground, and the brute force's time); the last wave of queries is a partial one."""
    pts = _cached("heap cloud", _heap_cloud)
    n = len(pts)
    assert n % 64 != 0
    heaps = _heap_ids(pts)
    assert [len(h) for h in heaps] == [m for _, m in HEAPS]
    up = pts[:, 2] > 5.0  # the heaps and the sparse points round them
    rng = np.random.default_rng(71)
    equal = np.where(up, f32(2.0), f32(0.0))  # every heap point 3, the sparse points round them 2, the slab 0
    for h in heaps:
        equal[h] = 3.0
    last = equal.copy()  # the largest score at each heap's last id
    for h in heaps:
        last[h[-1]] = 9.0
    edge = equal.copy()  # the only higher scores sit at exactly r from a heap, or strictly inside
    edge[n - 4:] = 5.0
    mixed = np.where(up, rng.integers(1, 4, n).astype(f32), f32(0.0))
    mixed[rng.random(n) < 0.01] = nan
    gone = np.concatenate([np.random.default_rng(9).choice(n - 4, n // 50, replace=False), [h[0] for h in heaps[:2]]])
    gone = np.unique(gone)
    plain = _cached(("heap sites", r), lambda: KO.sites(pts, r, only=up))
    groups = {None: plain, "deleted": KO.sites_without(plain, gone, n)}
    monkeypatch.setenv("PCGX_GRID", "2")
    t = kdtree.New(pts)
    _assert_heap_grid(t)
    td = kdtree.New(pts)
    td.DeletePoints(gone)
    for name, score in (("equal", equal), ("last", last), ("edge", edge), ("mixed", mixed)):
        want = KO.maxima_from_sites(score, groups[None])
        got = _maxima(t, r, score, (name, "grid"))
        assert np.array_equal(got, want), (name, r, np.setxor1d(got, want)[:10])
        monkeypatch.setenv("PCGX_RANGE_WALK", "1")
        assert np.array_equal(_maxima(t, r, score, (name, "walk")), want), (name, r)
        monkeypatch.delenv("PCGX_RANGE_WALK")
        wd = KO.maxima_from_sites(score, groups["deleted"])
        assert np.array_equal(_maxima(td, r, score, (name, "deleted")), wd), (name, r)
        assert not np.isin(wd, gone).any()
        _heap_expectations(name, r, n, heaps, want, wd, gone)


def _heap_expectations(name, r, n, heaps, want, wd, gone):
    """what the oracle's answer must look like at the heaps (no heap is within 1.0 of another)"""
    in_heap = [np.intersect1d(want, h).tolist() for h in heaps]
    first = [[int(h[0])] for h in heaps]
    if name == "equal":  # each heap keeps exactly its smallest id; its smallest id left after the deletions
        assert in_heap == first
        assert [np.intersect1d(wd, h).tolist() for h in heaps] == [[int(np.setdiff1d(h, gone)[0])] for h in heaps]
    if name == "last":  # only the last id survives in a heap
        assert in_heap == [[int(h[-1])] for h in heaps]
    if name == "edge":
        # a point at exactly DistSq == r^2 does not suppress its heap; one strictly inside does; one outside does not
        assert set(range(n - 4, n)) <= set(want.tolist())
        assert in_heap == (first[:2] + [[], []] if r == 1.0 else first)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_small_lengths(n):
    rng = np.random.default_rng(80 + n)
    pts = (rng.integers(0, 8, (n, 3)) / 8.0).astype(f32)
    s = _scores(n, 81)
    t = kdtree.New(pts)
    for r in (0.25, 0.13, 5.0):
        assert np.array_equal(_maxima(t, r, s, (n, r)), KO.local_maxima_direct(pts, s, r)), (n, r)


def test_compaction_tile_boundaries_and_nothing_found():
    tile = _compact_tile()
    for n in (tile - 1, tile, tile + 1, 3 * tile + 5):
        pts = np.ascontiguousarray(np.stack([np.arange(n), np.zeros(n), np.zeros(n)], axis=1), f32)
        pts = pts[np.random.default_rng(n).permutation(n)]
        t = kdtree.New(pts)
        ids, m = _raw(t, 0.5, np.ones(n, f32))  # every point alone in its neighbourhood
        assert m == n and np.array_equal(ids, np.arange(n))
        ids, m = _raw(t, 0.5, np.zeros(n, f32))
        assert m == 0 and np.all(ids == -1)
        s = np.ones(n, f32)
        s[::3] = nan
        assert np.array_equal(_maxima(t, 0.5, s), np.nonzero(~np.isnan(s))[0])


def test_bad_arguments():
    lib = L.lib()
    pts = synth.uniform_cloud(100, 1.0, 90)
    t = kdtree.New(pts)
    s = np.ones(100, f32)
    ids = np.zeros(100, np.int64)
    eig = np.zeros((100, 3), f32)
    cnt = C.c_int64(5)
    for r in (0.0, -1.0, inf, nan):
        assert lib.pcgx_kdtree_local_maxima(t._h, r, L.ptr(s), L.ptr(ids), C.byref(cnt)) == L.PCGX_E_INVALID
        assert lib.pcgx_kdtree_iss_keypoints(t._h, r, 0.1, 0.975, 0.975, 5, None, None, L.ptr(ids), C.byref(cnt)) == L.PCGX_E_INVALID
        assert lib.pcgx_kdtree_iss_keypoints(t._h, 0.1, r, 0.975, 0.975, 5, None, None, L.ptr(ids), C.byref(cnt)) == L.PCGX_E_INVALID
        assert lib.pcgx_kdtree_iss_keypoints(t._h, 0.1, 0.1, r, 0.975, 5, None, None, L.ptr(ids), C.byref(cnt)) == L.PCGX_E_INVALID
        assert lib.pcgx_kdtree_iss_keypoints(t._h, 0.1, 0.1, 0.975, r, 5, None, None, L.ptr(ids), C.byref(cnt)) == L.PCGX_E_INVALID
        assert lib.pcgx_kdtree_local_maxima_dev(t._h, r, L.ptr(s), L.ptr(ids), L.ptr(ids), None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_local_maxima(None, 0.1, L.ptr(s), L.ptr(ids), C.byref(cnt)) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_local_maxima(t._h, 0.1, None, L.ptr(ids), C.byref(cnt)) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_local_maxima(t._h, 0.1, L.ptr(s), None, C.byref(cnt)) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_local_maxima(t._h, 0.1, L.ptr(s), L.ptr(ids), None) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_iss_keypoints(None, 0.1, 0.1, 0.975, 0.975, 5, None, None, L.ptr(ids), C.byref(cnt)) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_iss_keypoints(t._h, 0.1, 0.1, 0.975, 0.975, 5, L.ptr(eig), None, None, C.byref(cnt)) == L.PCGX_E_INVALID
    assert lib.pcgx_kdtree_iss_keypoints(t._h, 0.1, 0.1, 0.975, 0.975, 5, L.ptr(eig), None, L.ptr(ids), None) == L.PCGX_E_INVALID
    assert cnt.value == 5
    # the optional outputs may be left out, one by one: the same ids
    want = t.ISSKeypoints(0.3, 0.2)[0]
    for e, sal in ((None, None), (L.ptr(eig), None), (None, L.ptr(s))):
        L.check(lib.pcgx_kdtree_iss_keypoints(t._h, 0.3, 0.2, 0.975, 0.975, 5, e, sal, L.ptr(ids), C.byref(cnt)))
        assert np.array_equal(ids[:cnt.value], want) and np.all(ids[cnt.value:] == -1)


# ------------------------------------------------------------------------------------------------ ISS

def _iss_case(name):
    def make():
        if name == "surface":
            pts = synth.surface_cloud(200_000, 30.0, 6)[0]
            t = kdtree.New(pts)
            offs, ids, _ = t.RangeBatch(pts, 0.1)  # (tests/test_gpu_kdtree.py pins Range to the C oracle)
            return [(pts, t, offs, ids)]
        out = []
        for pts in PO.moved_clouds():
            out.append((pts, kdtree.New(pts)) + KO.brute_lists(pts, 0.1))
        return out
    return _cached(("iss", name), make)


@pytest.mark.parametrize("name", ["moved", "surface"])
def test_iss_against_the_oracle(name):
    r = 0.1
    eigs, keys = [], []
    for pts, t, offs, ids in _iss_case(name):
        got_ids, eig, sal = t.ISSKeypoints(r, r)
        ref32, ref64, counts = KO.eigenvalues_from_lists(pts, offs, ids, 5)
        # accuracy: float32 rounding + the moments' bound (twice: the oracle rounds too)
        bound = KO.eigenvalue_bound(ref64, counts, r)
        err = np.abs(eig.astype(f64) - ref64)
        print(name, "eigenvalue error / bound: max %.3g" % float(np.max(err / bound)), "degenerate:", int((ref64[:, 2] == 0).sum()),
              "keypoints:", len(got_ids))
        assert np.all(err <= bound), (name, int(np.argmax(err / bound)), float(np.max(err / bound)))
        assert np.all(eig[ref64[:, 2] == 0] == 0) and (ref64[:, 2] > 0).sum() > len(pts) // 4
        assert np.all(eig[:, 0] >= 0) and np.all(eig[:, 0] <= eig[:, 1]) and np.all(eig[:, 1] <= eig[:, 2])
        # consistency: every decision after the eigenvalues, exactly
        assert np.array_equal(sal.view(u32), KO.saliency(eig, 0.975, 0.975).view(u32))
        assert np.array_equal(got_ids, t.LocalMaxima(r, sal))
        assert np.array_equal(got_ids, KO.maxima_from_lists(sal, offs, ids))
        eigs.append((eig, bound))
        keys.append(got_ids)
    if name == "moved":
        (ea, ba), (eb, bb) = eigs
        assert np.all(np.abs(ea.astype(f64) - eb.astype(f64)) <= 2.0 * np.maximum(ba, bb))
        assert len(keys[0]) > 30 and len(keys[1]) > 30
        # the pin's parameters (tests/test_keypoints_oracle.py): 51 keypoints by the float64 restatement
        for pts, t, _, _ in _iss_case(name):
            print("moved clouds at 0.15 / 0.1:", len(t.ISSKeypoints(0.15, 0.1)[0]), "keypoints")


def test_dev_forms_give_the_host_forms_bits():
    import torch
    dev = torch.device("cuda", 0)
    pts = synth.surface_cloud(20_000, 5.0, 33)[0]
    t = kdtree.New(pts)
    n = len(pts)
    want_ids, want_eig, want_sal = t.ISSKeypoints(0.15, 0.1)
    s = _scores(n, 34)
    want_max = t.LocalMaxima(0.1, s)
    assert len(want_ids) > 20 and len(want_max) > 20
    de, ds = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    di, dc = torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((1,), -7, dtype=torch.int32, device=dev)
    di2, dc2 = torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((1,), -7, dtype=torch.int32, device=dev)
    dscore = torch.from_numpy(s).to(dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        # one call (eigenvalue stage plus suppression plus compaction), then two more in a row on the same stream
        t.ISSKeypointsDev(0.15, 0.1, di.data_ptr(), dc.data_ptr(), de.data_ptr(), ds.data_ptr(), stream=st)
        stream.synchronize()
        m = int(dc.cpu()[0])
        got = di.cpu().numpy()
        assert m == len(want_ids) and np.array_equal(got[:m], want_ids) and np.all(got[m:] == -1)
        assert np.array_equal(de.cpu().numpy().view(u32), want_eig.view(u32))
        assert np.array_equal(ds.cpu().numpy().view(u32), want_sal.view(u32))
        t.LocalMaximaDev(0.1, dscore.data_ptr(), di2.data_ptr(), dc2.data_ptr(), stream=st)
        t.ISSKeypointsDev(0.15, 0.1, di.data_ptr(), dc.data_ptr(), stream=st)  # (no optional outputs)
        stream.synchronize()
    m2 = int(dc2.cpu()[0])
    got2 = di2.cpu().numpy()
    assert m2 == len(want_max) and np.array_equal(got2[:m2], want_max) and np.all(got2[m2:] == -1)
    assert int(dc.cpu()[0]) == m and np.array_equal(di.cpu().numpy(), got)


def test_device_chain_over_keypoints():
    """NormalsDev, FPFHDev and ISSKeypointsDev on both moved clouds on one stream, one read of the two counts, the
    keypoints' descriptor rows and points gathered with torch, CorrespondencesDev over them, EstimatePoseDev."""
    import torch
    P, P2 = PO.moved_clouds()
    r, vp, vp2 = 0.1, (0.8, 0.8, 50.0), (-0.8 + 2.25, 0.8 - 0.5, 50.0 + 1.75)
    t, t2 = kdtree.New(P), kdtree.New(P2)
    n, n_hyp, max_dist = len(P), 2048, 0.01
    dev = torch.device("cuda", 0)
    samples = alignment.Samples(n_hyp, 3)

    def buf(shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=dev)

    dP, dP2 = torch.from_numpy(P).to(dev), torch.from_numpy(P2).to(dev)
    du = torch.from_numpy(samples.view(np.int32)).to(dev)
    dn, dn2, df, df2 = buf((n, 3)), buf((n, 3)), buf((n, 33)), buf((n, 33))
    dk, dk2, counts = buf(n, torch.int32), buf(n, torch.int32), torch.full((2,), -1, dtype=torch.int32, device=dev)
    res = buf(alignment.RESULT_WORDS, torch.int32)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()  # torch's gathers and the library's kernels in one queue
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        t.NormalsDev(r, dn.data_ptr(), Viewpoint=vp, stream=st)
        t.FPFHDev(r, dn.data_ptr(), df.data_ptr(), stream=st)
        t.ISSKeypointsDev(0.15, 0.1, dk.data_ptr(), counts.data_ptr(), stream=st)
        t2.NormalsDev(r, dn2.data_ptr(), Viewpoint=vp2, stream=st)
        t2.FPFHDev(r, dn2.data_ptr(), df2.data_ptr(), stream=st)
        t2.ISSKeypointsDev(0.15, 0.1, dk2.data_ptr(), counts.data_ptr() + 4, stream=st)
        na, nb = (int(x) for x in counts.cpu().numpy())  # the one read (a copy on the same stream, waited for)
        assert 30 < na <= n and 30 < nb <= n, (na, nb)
        ka, kb = dk[:na].long(), dk2[:nb].long()
        fa, fb = df[ka].contiguous(), df2[kb].contiguous()
        pa, pb = dP[ka].contiguous(), dP2[kb].contiguous()
        src, dst, cnt = buf(na, torch.int32), buf(na, torch.int32), buf(1, torch.int32)
        features.CorrespondencesDev(fa.data_ptr(), na, fb.data_ptr(), nb, src.data_ptr(), dst.data_ptr(), cnt.data_ptr(),
                                    MaxRatio=1.0, Mutual=True, stream=st)
        alignment.EstimatePoseDev(pa.data_ptr(), na, pb.data_ptr(), nb, src.data_ptr(), dst.data_ptr(), na, du.data_ptr(),
                                  n_hyp, res.data_ptr(), max_dist, d_n_pairs=cnt.data_ptr(), stream=st)
        stream.synchronize()
    torch.cuda.synchronize()
    got = alignment.ReadResult(res.cpu().numpy())
    print("keypoints: %d and %d, pairs: %d, inliers: %d" % (na, nb, int(cnt.cpu().numpy()[0]), got["n_inliers"]))
    assert got["found"]
    assert np.max(np.linalg.norm(mat.Transform(got["pose"], P).astype(f64) - P2, axis=1)) < max_dist
