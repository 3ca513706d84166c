"""FPFH matching on the GPU (pcgx_fpfh_match / _correspondences / _dev, csrc/fpfh_match.hip) against the NumPy oracle
(tests/match_oracle.py).  Everything is compared for EQUALITY: ids as integers, distances as uint32 views -- scene R is
decisive for that (tests/test_match_oracle.py: no tie between best and runner-up, and a fused, widened or reordered
sum has other bits in a third of the queries and more).  PCGX_MATCH_SPLIT forces the number of chunks of B so that the
merge of the chunks' results runs at these small shapes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import features, kdtree, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_oracle as MO  # noqa: E402
from test_match_oracle import hand_cases, scene_r_reference  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64, u32 = np.float32, np.float64, np.uint32
INF = f32(np.inf)

_CACHE = {}


def _cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _split(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("PCGX_MATCH_SPLIT", raising=False)
    else:
        monkeypatch.setenv("PCGX_MATCH_SPLIT", str(split))


def _ratio_sq(ratio):
    r = f32(ratio)
    return r * r  # what Correspondences passes: float32(MaxRatio)^2, a float32 product


def _same_match(got, want, what):
    ids, d1, d2 = got
    assert ids.dtype == np.int64 and d1.dtype == f32 and d2.dtype == f32, what
    bad = np.nonzero(ids != want[0])[0]
    assert len(bad) == 0, (what, "ids", bad[:5], ids[bad[:5]], want[0][bad[:5]])
    for name, g, w in (("dist_sq", d1, want[1]), ("second_dist_sq", d2, want[2])):
        bad = np.nonzero(g.view(u32) != w.view(u32))[0]
        assert len(bad) == 0, (what, name, bad[:5], g[bad[:5]], w[bad[:5]])


def _check_all(A, B, what, ratios=(1.0, 0.9)):
    """Match and Correspondences (every ratio, mutual on and off) of A in B against the oracle"""
    D = MO.dist_matrix(A, B)
    ua, ub = MO.usable(A), MO.usable(B)
    want = MO.match_from(D, ua, ub)
    _same_match(features.Match(A, B), want, what)
    back = MO.match_from(np.ascontiguousarray(D.T), ub, ua)[0]
    for ratio in ratios:
        for mutual in (True, False):
            w = MO.correspondences_from_matches(*want, back, _ratio_sq(ratio), mutual)
            g = features.Correspondences(A, B, ratio, mutual)
            assert g.dtype == np.int64 and np.array_equal(g, w), (what, ratio, mutual, len(g), len(w))
    return want


# ------------------------------------------------------------------------------------------------ scene R

def _scene_r_wants():
    R = scene_r_reference()
    back = MO.match_from(np.ascontiguousarray(R["D"].T), MO.usable(R["B"]), MO.usable(R["A"]))[0]
    out = {}
    for ratio in (1.0, 0.9):
        for mutual in (True, False):
            out[ratio, mutual] = MO.correspondences_from_matches(R["ids"], R["d1"], R["d2"], back, _ratio_sq(ratio), mutual)
    return out


@pytest.mark.parametrize("split", [None, 1, 2, 3, 7])
def test_scene_r(split, monkeypatch):
    R = scene_r_reference()
    A, B = R["A"], R["B"]
    assert len(A) % 64 == 56 and len(B) % 2 == 1 and len(A) > 2 * features.MatchTile()
    wants = _cached("scene R correspondences", _scene_r_wants)
    # the four lists differ from each other, and none is empty or everything
    sizes = sorted(len(w) for w in wants.values())
    assert 0 < sizes[0] < sizes[1] < sizes[2] < sizes[3] == len(A)
    _split(monkeypatch, split)
    _same_match(features.Match(A, B), (R["ids"], R["d1"], R["d2"]), "scene R, split %s" % split)
    for (ratio, mutual), w in wants.items():
        g = features.Correspondences(A, B, ratio, mutual)
        assert np.array_equal(g, w), (split, ratio, mutual, len(g), len(w))


@pytest.mark.parametrize("split", [None, 1, 300])
def test_shape_sweep(split, monkeypatch):
    """every small shape round the wave and the tile, rows of scene R (its distance matrix's corner is theirs); 300
    chunks are more than B has rows: most are empty"""
    R = scene_r_reference()
    _split(monkeypatch, split)
    for na in (1, 63, 64, 65, 130):
        for nb in (1, 2, 63, 64, 65, 257):
            A, B = R["A"][:na], R["B"][:nb]
            D = R["D"][:na, :nb]
            ones_a, ones_b = np.ones(na, bool), np.ones(nb, bool)
            want = MO.match_from(D, ones_a, ones_b)
            what = "%d x %d, split %s" % (na, nb, split)
            got = features.Match(A, B)
            _same_match(got, want, what)
            assert np.all(got[0] >= 0)
            if nb == 1:
                assert np.all(np.isposinf(got[2])) and np.all(got[0] == 0)
            else:
                assert np.all(got[2] > got[1])
            for ratio, mutual in ((1.0, True), (0.9, False)):
                w = MO.correspondences_from(D, ones_a, ones_b, _ratio_sq(ratio), mutual)
                assert np.array_equal(features.Correspondences(A, B, ratio, mutual), w), (what, ratio, mutual)


# ------------------------------------------------------------------------------------------------ ties

def _tie_scene():
    """B: 500 distinct rows of integers in {0 .. 3}, each three times, at ids scattered by a permutation (every D is an
    exact integer <= 297 in any evaluation order: only the tie rule is under test).  A: 350 copies of rows of B (three
    candidates at D = 0) and 350 rows of B with one value changed to another of {0 .. 3} (three candidates at D = 1, 4
    or 9; every other row is far).  -> A, B, base (the row of the 500 each query was made from), where (its ids in B)"""
    rng = np.random.default_rng(99)
    rows = rng.integers(0, 4, (500, MO.LEN)).astype(f32)
    assert len(np.unique(rows, axis=0)) == 500
    perm = rng.permutation(1500)
    B = np.ascontiguousarray(np.repeat(rows, 3, axis=0)[perm])
    where = np.argsort(perm, kind="stable").reshape(500, 3)  # where[r] = the ids of row r's three copies
    where.sort(axis=1)
    base = rng.integers(0, 500, 700)
    A = rows[base].copy()
    col = rng.integers(0, MO.LEN, 350)
    A[350 + np.arange(350), col] = (A[350 + np.arange(350), col] + rng.integers(1, 4, 350)) % 4
    order = rng.permutation(700)
    return np.ascontiguousarray(A[order]), B, base[order], where


@pytest.mark.parametrize("split", [1, 2, 3, 7])
def test_ties_go_to_the_smaller_id(split, monkeypatch):
    A, B, base, where = _cached("ties", _tie_scene)
    want = _cached("ties ref", lambda: MO.match(A, B))
    # by construction: best and runner-up tie in every query, the id is the smallest of the three copies
    assert np.array_equal(want[1], want[2]) and np.array_equal(want[0], where[base, 0])
    assert (want[1] == 0).sum() == 350 and set(np.unique(want[1])) == {0.0, 1.0, 4.0, 9.0}
    # ... and the three tied ids fall in different chunks of B at the splits > 1
    if split == 7:
        chunk = (len(B) + 6) // 7
        assert np.mean(where[base, 0] // chunk != where[base, 1] // chunk) > 0.5
    _split(monkeypatch, split)
    got = features.Match(A, B)
    _same_match(got, want, "ties, split %d" % split)
    assert np.array_equal(features.Correspondences(A, B, 1.0, False)[:, 0], np.arange(len(A)))
    lower = features.Correspondences(A, B, 0.999, False)  # D1 == D2: any ratio below 1 keeps D1 == 0 alone
    assert np.array_equal(lower[:, 0], np.nonzero(want[1] == 0)[0])
    D = _cached("ties D", lambda: MO.dist_matrix(A, B))
    ones_a, ones_b = np.ones(len(A), bool), np.ones(len(B), bool)
    for ratio in (1.0, 0.999):
        w = _cached(("ties corr", ratio), lambda: MO.correspondences_from(D, ones_a, ones_b, _ratio_sq(ratio), True))
        assert np.array_equal(features.Correspondences(A, B, ratio, True), w)
    assert 0 < len(_cached(("ties corr", 1.0), None)) < len(A)


def test_ratio_test_is_less_or_equal():
    """D1 = 1, D2 = 4 and max_ratio_sq = 0.25 exactly (MaxRatio 0.5): kept, the rule is <="""
    A = np.zeros((1, MO.LEN), f32)
    A[0, 7] = 1.0
    B = np.zeros((2, MO.LEN), f32)
    B[0, 7] = 3.0
    B[1, 7] = 2.0
    ids, d1, d2 = features.Match(A, B)
    assert (ids[0], d1[0], d2[0]) == (1, 1.0, 4.0)
    for mutual in (False, True):
        assert features.Correspondences(A, B, 0.5, mutual).tolist() == [[0, 1]]
        assert features.Correspondences(A, B, 0.4999, mutual).tolist() == []


# ------------------------------------------------------------------------------------------------ unusable rows

def _spoil(rows, at):
    """zero, -0.0, one-NaN and one-inf rows at the positions `at`, the kinds in turn"""
    rows = rows.copy()
    for k, i in enumerate(at):
        kind = k % 4
        if kind == 0:
            rows[i] = 0.0
        elif kind == 1:
            rows[i] = -0.0
        elif kind == 2:
            rows[i, (5 * k) % MO.LEN] = np.nan
        else:
            rows[i, (7 * k) % MO.LEN] = np.inf if k % 8 == 3 else -np.inf
    return rows


@pytest.mark.parametrize("split", [None, 3])
def test_unusable_rows(split, monkeypatch):
    R = scene_r_reference()
    T = features.MatchTile()
    assert T >= 64 and T % 64 == 0
    n = 2 * T + 45
    spots = sorted({0, 63, 64, T - 1, T, n - 1})
    _split(monkeypatch, split)
    for rot_a, rot_b in ((0, 0), (1, 2), (2, 3), (3, 1)):  # every kind of row at every spot, in A and in B
        A = _spoil(R["A"][:n], np.roll(spots, rot_a))
        B = _spoil(R["B"][:n], np.roll(spots, rot_b))
        assert (~MO.usable(A)).sum() == len(spots) == (~MO.usable(B)).sum()
        want = _check_all(A, B, "unusable rows %d %d, split %s" % (rot_a, rot_b, split))
        assert np.all(want[0][spots] == -1) and not np.isin(want[0], spots).any()
    # the nearest row of a query made unusable: the runner-up moves up
    A, B = R["A"][:n].copy(), R["B"][:n].copy()
    first = MO.match(A, B)
    second_id = np.argsort(R["D"][:n, :n], axis=1, kind="stable")[:, 1]
    B[first[0][:T]] = 0.0
    want = _check_all(A, B, "nearest rows zeroed")
    moved = np.nonzero(~np.isin(second_id[:T], first[0][:T]))[0]  # (whose runner-up was not zeroed as well)
    assert len(moved) > T // 4 and np.array_equal(want[0][moved], second_id[moved])
    assert np.array_equal(want[1][moved].view(u32), first[2][moved].view(u32))
    # B without a usable row, and with exactly one (behind the first tile)
    B0 = _spoil(R["B"][:n], np.arange(n))
    assert not MO.usable(B0).any()
    got = features.Match(A, B0)
    assert np.all(got[0] == -1) and np.all(np.isposinf(got[1])) and np.all(np.isposinf(got[2]))
    assert len(features.Correspondences(A, B0)) == 0
    B1 = B0.copy()
    B1[T + 3] = R["B"][T + 3]
    want = _check_all(A, B1, "one usable candidate")
    assert np.all(want[0] == T + 3) and np.all(np.isposinf(want[2])) and np.all(np.isfinite(want[1]))
    # rows of +-1e20 are usable, but at D = +inf of everything else: unmatched as queries, never a match or a runner-up
    # as candidates -- except of each other (D = 0)
    A2, B2 = R["A"][:n].copy(), R["B"][:n].copy()
    A2[[0, 64, n - 1]] = 1e20
    A2[5] = -1e20
    B2[[1, T, n - 2]] = -1e20
    want = _check_all(A2, B2, "1e20 rows")
    assert np.all(want[0][[0, 64, n - 1]] == -1) and want[0][5] == 1 and want[1][5] == 0 and want[2][5] == 0
    for name, A3, B3, ids, d1, d2 in hand_cases():  # the rows worked by hand (tests/test_match_oracle.py)
        _same_match(features.Match(A3, B3), (np.array(ids, np.int64), np.array(d1, f32), np.array(d2, f32)), name)


# ------------------------------------------------------------------------------------------------ real descriptors

def test_self_match():
    """descriptors the library made: every usable row finds itself or an identical row before it at D = 0; the 20
    isolated points have zero rows and are unmatched"""
    P0, N0 = synth.surface_cloud(3000, 1.65, 6)
    far = (np.arange(20, dtype=f32)[:, None] * f32(2.0) + f32(10.0)) * np.ones((1, 3), f32)
    P = np.ascontiguousarray(np.concatenate([P0, far]), f32)
    N = np.ascontiguousarray(np.concatenate([N0, np.tile(np.array([0, 0, 1], f32), (20, 1))]), f32)
    f = kdtree.New(P).FPFH(0.1, N)[0]
    ok = MO.usable(f)
    assert not ok[-20:].any() and np.all(f[-20:] == 0) and ok[:3000].sum() > 2900
    ids, d1, d2 = features.Match(f, f)
    firsts = {}
    for i in np.nonzero(ok)[0]:
        firsts.setdefault((f[i] + f32(0.0)).tobytes(), i)
    want = np.array([firsts[(f[i] + f32(0.0)).tobytes()] if ok[i] else -1 for i in range(len(f))], np.int64)
    assert np.array_equal(ids, want)
    assert np.all(d1[ok] == 0) and np.all(np.isposinf(d1[~ok])) and np.all(np.isposinf(d2[~ok]))
    assert np.all(d2[ok] >= 0) and np.all(np.isfinite(d2[ok]))
    c = features.Correspondences(f, f)
    assert np.array_equal(c[:, 0], c[:, 1]) and np.array_equal(c[:, 0], np.nonzero(ids == np.arange(len(f)))[0])


def _moved_clouds():
    """the two clouds of tests/test_gpu_fpfh.py::test_exact_rigid_motion (the recipe, copied): a cloud on the 2^-10
    lattice, and the same turned by 90 degrees about z and shifted by multiples of 1/4"""
    rng = np.random.default_rng(77)
    xy = rng.integers(0, 1690, (3000, 2)).astype(f64) / 1024.0
    x, y = xy[:, 0], xy[:, 1]
    z = np.rint((0.5 * np.sin(0.7 * x) * np.cos(0.5 * y) + 0.3 * np.sin(1.3 * y)) * 1024.0) / 1024.0
    P = np.ascontiguousarray(np.stack([x, y, z], axis=1), f32)
    P2 = np.ascontiguousarray(np.stack([-P[:, 1], P[:, 0], P[:, 2]], axis=1) + np.array([2.25, -0.5, 1.75], f32), f32)
    return P, P2


def test_device_chain():
    """NormalsDev -> FPFHDev -> MatchDev / CorrespondencesDev on one stream, nothing copied to the host in between:
    the host entry points' bits, the oracle's on the library's descriptors, and the same bits twice"""
    import torch
    P, P2 = _moved_clouds()
    r, vp, vp2 = 0.1, (0.8, 0.8, 50.0), (-0.8 + 2.25, 0.8 - 0.5, 50.0 + 1.75)
    t, t2 = kdtree.New(P), kdtree.New(P2)
    n = len(P)
    dev = torch.device("cuda", 0)

    def buf(shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=dev)

    runs = []
    for _ in range(2):
        dn, dn2, df, df2 = buf((n, 3)), buf((n, 3)), buf((n, 33)), buf((n, 33))
        ids, d1, d2 = buf(n, torch.int32), buf(n), buf(n)
        src, dst, cnt = buf(n, torch.int32), buf(n, torch.int32), buf(1, torch.int32)
        torch.cuda.synchronize()
        st = torch.cuda.current_stream().cuda_stream
        t.NormalsDev(r, dn.data_ptr(), Viewpoint=vp, stream=st)
        t.FPFHDev(r, dn.data_ptr(), df.data_ptr(), stream=st)
        t2.NormalsDev(r, dn2.data_ptr(), Viewpoint=vp2, stream=st)
        t2.FPFHDev(r, dn2.data_ptr(), df2.data_ptr(), stream=st)
        features.MatchDev(df.data_ptr(), n, df2.data_ptr(), n, ids.data_ptr(), d1.data_ptr(), d2.data_ptr(), stream=st)
        features.CorrespondencesDev(df.data_ptr(), n, df2.data_ptr(), n, src.data_ptr(), dst.data_ptr(), cnt.data_ptr(),
                                    MaxRatio=0.95, Mutual=True, stream=st)
        torch.cuda.synchronize()
        runs.append([x.cpu().numpy() for x in (df, df2, ids, d1, d2, src, dst, cnt)])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(u32), b.view(u32))
    f, f2, ids, d1, d2, src, dst, cnt = runs[0]
    # the host entry points on the host's copy of the same chain
    hf = t.FPFH(r, t.Normals(r, Viewpoint=vp)[0])[0]
    hf2 = t2.FPFH(r, t2.Normals(r, Viewpoint=vp2)[0])[0]
    assert np.array_equal(hf.view(u32), f.view(u32)) and np.array_equal(hf2.view(u32), f2.view(u32))
    assert MO.usable(f).sum() > 2900
    want = _check_all(hf, hf2, "moved clouds", ratios=(1.0, 0.95))
    assert ids.dtype == np.int32 and src.dtype == np.int32
    _same_match((ids.astype(np.int64), d1, d2), want, "MatchDev")
    m = int(cnt[0])
    c = features.Correspondences(hf, hf2, 0.95, True)
    assert m == len(c) and np.array_equal(src[:m], c[:, 0]) and np.array_equal(dst[:m], c[:, 1])
    assert np.all(src[m:] == -1) and np.all(dst[m:] == -1) and 0 < m < n
    # MatchDev without the runner-up's distance
    ids2, e1 = buf(n, torch.int32), buf(n)
    features.MatchDev(df.data_ptr(), n, df2.data_ptr(), n, ids2.data_ptr(), e1.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(ids2.cpu().numpy(), ids) and np.array_equal(e1.cpu().numpy().view(u32), d1.view(u32))
    # recorded in DESIGN.md 3.11, not asserted: how many mutual correspondences name the moved copy of their own point
    allc = features.Correspondences(hf, hf2, 1.0, True)
    print("moved clouds: %d mutual correspondences of %d points, dst == src in %d (%.1f %%); at MaxRatio 0.95: %d, %d (%.1f %%)"
          % (len(allc), n, int((allc[:, 0] == allc[:, 1]).sum()), 100.0 * np.mean(allc[:, 0] == allc[:, 1]),
             m, int((c[:, 0] == c[:, 1]).sum()), 100.0 * np.mean(c[:, 0] == c[:, 1])))


# ------------------------------------------------------------------------------------------------ arguments

def test_bad_arguments_and_empty_inputs():
    R = scene_r_reference()
    A, B = np.ascontiguousarray(R["A"][:70]), np.ascontiguousarray(R["B"][:50])
    lib = L.lib()
    na, nb = len(A), len(B)
    ids, src, dst, cnt = (np.full(na, 7, np.int64) for _ in range(4))
    d1, d2 = np.full(na, 7, f32), np.full(na, 7, f32)
    p = L.ptr
    E, OK = L.PCGX_E_INVALID, L.PCGX_OK
    x = C.c_void_p(16)  # (a device address nobody reads: the arguments are refused first)
    # NULL arrays, negative counts
    assert lib.pcgx_fpfh_match(None, na, p(B), nb, p(ids), p(d1), p(d2)) == E
    assert lib.pcgx_fpfh_match(p(A), na, None, nb, p(ids), p(d1), p(d2)) == E
    assert lib.pcgx_fpfh_match(p(A), na, p(B), nb, None, p(d1), p(d2)) == E
    assert lib.pcgx_fpfh_match(p(A), na, p(B), nb, p(ids), None, p(d2)) == E
    assert lib.pcgx_fpfh_match(p(A), -1, p(B), nb, p(ids), p(d1), p(d2)) == E
    assert lib.pcgx_fpfh_match(p(A), na, p(B), -1, p(ids), p(d1), p(d2)) == E
    assert lib.pcgx_fpfh_match_dev(None, na, x, nb, x, x, x, None) == E
    assert lib.pcgx_fpfh_match_dev(x, na, None, nb, x, x, x, None) == E
    assert lib.pcgx_fpfh_match_dev(x, na, x, nb, None, x, x, None) == E
    assert lib.pcgx_fpfh_match_dev(x, na, x, nb, x, None, x, None) == E
    assert lib.pcgx_fpfh_match_dev(x, -1, x, nb, x, x, x, None) == E
    assert lib.pcgx_fpfh_match_dev(x, na, x, -1, x, x, x, None) == E
    assert np.all(ids == 7) and np.all(d1 == 7)
    for a_, b_, s_, d_, c_ in ((None, p(B), p(src), p(dst), p(cnt)), (p(A), None, p(src), p(dst), p(cnt)),
                               (p(A), p(B), None, p(dst), p(cnt)), (p(A), p(B), p(src), None, p(cnt)),
                               (p(A), p(B), p(src), p(dst), None)):
        assert lib.pcgx_fpfh_correspondences(a_, na, b_, nb, 1.0, 1, s_, d_, c_) == E
    for a_, b_, s_, d_, c_ in ((None, x, x, x, x), (x, None, x, x, x), (x, x, None, x, x), (x, x, x, None, x), (x, x, x, x, None)):
        assert lib.pcgx_fpfh_correspondences_dev(a_, na, b_, nb, 1.0, 1, s_, d_, c_, None) == E
    assert lib.pcgx_fpfh_correspondences(p(A), -1, p(B), nb, 1.0, 1, p(src), p(dst), p(cnt)) == E
    assert lib.pcgx_fpfh_correspondences(p(A), na, p(B), -1, 1.0, 1, p(src), p(dst), p(cnt)) == E
    # the ratio: 0 < max_ratio_sq <= 1 and finite
    for bad in (0.0, -0.5, 1.0000001, 2.0, float("inf"), float("nan")):
        assert lib.pcgx_fpfh_correspondences(p(A), na, p(B), nb, bad, 1, p(src), p(dst), p(cnt)) == E
        assert lib.pcgx_fpfh_correspondences_dev(x, na, x, nb, bad, 1, x, x, x, None) == E
        assert lib.pcgx_fpfh_correspondences(p(A), 0, p(B), nb, bad, 1, p(src), p(dst), p(cnt)) == E
    assert np.all(src == 7) and np.all(cnt == 7)
    with pytest.raises(ValueError):
        features.Match(A[:, :32], B)
    with pytest.raises(L.PcgxError):
        features.Correspondences(A, B, MaxRatio=1.5)
    # na == 0: PCGX_OK, nothing written except *n_pairs = 0 (NULL arrays are fine then)
    assert lib.pcgx_fpfh_match(None, 0, p(B), nb, None, None, None) == OK
    assert lib.pcgx_fpfh_match_dev(None, 0, None, 0, None, None, None, None) == OK
    assert lib.pcgx_fpfh_correspondences(None, 0, p(B), nb, 1.0, 1, p(src), p(dst), p(cnt)) == OK
    assert cnt[0] == 0 and np.all(cnt[1:] == 7) and np.all(src == 7) and np.all(dst == 7)
    assert lib.pcgx_fpfh_correspondences(None, 0, None, 0, 1.0, 0, None, None, None) == OK
    e = np.zeros((0, 33), f32)
    got = features.Match(e, B)
    assert all(len(a) == 0 for a in got) and features.Correspondences(e, B).shape == (0, 2)
    # nb == 0: PCGX_OK, every query unmatched (NULL b is fine then)
    assert lib.pcgx_fpfh_match(p(A), na, None, 0, p(ids), p(d1), p(d2)) == OK
    assert np.all(ids == -1) and np.all(np.isposinf(d1)) and np.all(np.isposinf(d2))
    for mutual in (0, 1):
        src[:] = 7
        assert lib.pcgx_fpfh_correspondences(p(A), na, None, 0, 1.0, mutual, p(src), p(dst), p(cnt)) == OK
        assert cnt[0] == 0 and np.all(src == -1) and np.all(dst == -1)
    # the runner-up's distance may be left out; two runs give the same bits
    assert lib.pcgx_fpfh_match(p(A), na, p(B), nb, p(ids), p(d1), None) == OK
    g = features.Match(A, B)
    g2 = features.Match(A, B)
    assert np.array_equal(ids, g[0]) and np.array_equal(d1.view(u32), g[1].view(u32))
    for a, b in zip(g, g2):
        assert np.array_equal(a.view(u32) if a.dtype == f32 else a, b.view(u32) if b.dtype == f32 else b)
    assert np.array_equal(features.Correspondences(A, B, 0.9), features.Correspondences(A, B, 0.9))
    # the -1 tail behind the pairs
    assert lib.pcgx_fpfh_correspondences(p(A), na, p(B), nb, 1.0, 1, p(src), p(dst), p(cnt)) == OK
    m = int(cnt[0])
    assert 0 < m < na and np.all(src[m:] == -1) and np.all(dst[m:] == -1) and np.all(src[:m] >= 0) and np.all(np.diff(src[:m]) > 0)
