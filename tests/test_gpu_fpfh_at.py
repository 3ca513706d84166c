"""FPFH at chosen points (pcgx_kdtree_fpfh_at / _dev, csrc/fpfh.hip) against two yardsticks: the float64 oracle
(tests/fpfh_oracle.py) on scenes that have no fragile pair (tests/test_fpfh_oracle.py: the count checks are
equalities, nothing is left out of the float check), and the full call on the same handle, whose rows at the ids the
compact rows must equal BIT FOR BIT -- the third stage sums a query's neighbourhood in the order fpfh_kernel's lane
takes for that point (csrc/fpfh.hip), so equality is asserted instead of the 2^-21 (1 + 2^-20) max(|a|, |b|) that two
values within 2^-22 of one real number are bound to.  n_spfh, the number of points whose SPFH record the call
computed, must equal the size of the union of the selected points and their neighbourhoods by brute force in float32:
the proof, without a clock, that the rest of the cloud was left alone."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import alignment, features, kdtree, mat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_oracle as FO  # noqa: E402
import normals_oracle as NO  # noqa: E402
import pose_oracle as PO  # noqa: E402
import test_gpu_fpfh as TF  # noqa: E402
from test_gpu_radius_edges import _assert_heap_grid, _grid_on  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64, u32 = np.float32, np.float64, np.uint32

_CACHE = {}


def _cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _rows(ref, ids):
    """the oracle's result for the whole cloud (FO.fpfh over all points) -> the same for the rows `ids`"""
    nq = len(ref["pairs"])
    out = {k: v[ids] for k, v in ref.items() if isinstance(v, np.ndarray) and len(v) == nq}
    out["n_valid"] = int(out["m_lo"].sum())
    out["n_fragile"] = int(out["fragile"].sum())
    assert out["n_fragile"] == 0 and out["float_ok"].all()  # nothing is left out of the float check on these scenes
    return out


def _union(P, ids, r, deleted=None):
    """how many distinct points are a selected point or inside the radius of one: float32 DistSq < r * r by brute
    force (a deleted point is nobody's neighbour, but a selected one has a record of its own)"""
    pts = np.array(P, f32)
    if deleted is not None:
        pts[deleted] = np.nan
    bound = f32(r) * f32(r)
    need = np.zeros(len(P), bool)
    for i in np.unique(ids):
        need |= NO.dist_sq_f32(pts, P[i]) < bound
        need[i] = True
    return int(need.sum())


def _bits(a):
    return np.ascontiguousarray(a).view(u32)


def _check_against_full(got, full, P, ids, what):
    """the compact outputs against the full call's rows at the ids: bit for bit"""
    f, x, c, m, _ = got
    ff, fc, fm = full
    assert np.array_equal(_bits(f), _bits(ff[ids])), what
    assert np.array_equal(c, fc[ids]) and np.array_equal(m, fm[ids]), what
    assert np.array_equal(_bits(x), _bits(P[ids])), what


# ------------------------------------------------------------------------------------------------ the surface

def _surface():
    """the surface scene with one point moved far away (isolated: m == 0, a zero row) and one normal zeroed"""
    def make():
        P0, N0, r = TF._scene("surface")
        P, N = P0.copy(), N0.copy()
        P[17] = (40.0, 40.0, 40.0)
        N[1234] = 0
        ref = TF._oracle_all(P, N, r)
        assert ref["n_fragile"] == 0 and np.array_equal(ref["lo"], ref["hi"]) and ref["float_ok"].all()
        gone = np.random.default_rng(5).choice(len(P), len(P) // 10, replace=False)
        refd = TF._oracle_all(P, N, r, gone)
        assert refd["n_fragile"] == 0 and refd["float_ok"].all()
        return dict(P=P, N=N, r=r, ref=ref, gone=gone, refd=refd, isolated=17, zero_normal=1234)
    return _cached("surface", make)


def _id_sets(sc, t):
    rng = np.random.default_rng(99)
    n = len(sc["P"])
    sets = {"n%d" % k: rng.choice(n, k, replace=False) for k in (1, 63, 64, 65, 129)}
    sets["duplicates, descending"] = np.sort(np.concatenate([rng.choice(n, 40, replace=False)] * 3))[::-1]
    sets["a deleted id"] = np.concatenate([sc["gone"][:3], rng.choice(n, 30, replace=False)])
    sets["isolated"] = np.array([sc["isolated"]])
    sets["zero normal"] = np.concatenate([[sc["zero_normal"]], rng.choice(n, 9, replace=False)])
    sets["iss"] = t.ISSKeypoints(sc["r"], sc["r"])[0]
    return {k: np.ascontiguousarray(v, np.int64) for k, v in sets.items()}


@pytest.mark.parametrize("handle", ["grid", "walk", "deleted"])
def test_surface_id_sets_on_every_kind_of_handle(handle, monkeypatch):
    sc = _surface()
    P, N, r = sc["P"], sc["N"], sc["r"]
    t = kdtree.New(P)
    gone = None
    if handle == "deleted":
        gone = sc["gone"]
        t.DeletePoints(gone)
    if handle == "walk":
        monkeypatch.setenv("PCGX_RANGE_WALK", "1")
    ref = sc["refd"] if handle == "deleted" else sc["ref"]
    full = t.FPFH(r, N)
    FO.check(ref, *full, what="full call, " + handle)
    sets = _id_sets(sc, t)
    assert len(sets["iss"]) > 10
    for name, ids in sets.items():
        what = "%s, %s" % (name, handle)
        got = t.FPFHAt(r, N, ids)
        f, x, c, m, n_spfh = got
        if name != "isolated":  # (the oracle's check wants a valid pair to look at; the isolated point is checked below)
            FO.check(_rows(ref, ids), f, c, m, what=what)
        _check_against_full(got, full, P, ids, what)
        want = _union(P, ids, r, gone)
        print(what, "n_spfh", n_spfh, "of", len(P))
        assert n_spfh == want, (what, n_spfh, want)
        if len(ids) <= 129:
            assert n_spfh < len(P), what
    # the isolated point: a zero row, and the only record computed
    f, x, c, m, n_spfh = t.FPFHAt(r, N, sets["isolated"])
    assert n_spfh == 1 and m[0] == 0 and np.all(c == 0) and np.all(_bits(f) == 0)
    assert np.array_equal(x[0], f32([40.0, 40.0, 40.0]))
    # the point whose own normal is zero: no pair of its own, the neighbours' term alone (100 per feature)
    f, x, c, m, _ = t.FPFHAt(r, N, sets["zero normal"][:1])
    assert m[0] == 0 and np.all(c == 0) and np.all(np.abs(f.astype(f64).reshape(3, 11).sum(axis=1) - 100.0) <= 1e-4)


def test_sphere():
    P, N, r = TF._scene("sphere")
    ref = _cached("sphere ref", lambda: TF._oracle_all(P, N, r))
    assert ref["n_fragile"] == 0 and ref["float_ok"].all()
    t = kdtree.New(P)
    full = t.FPFH(r, N)
    ids = np.random.default_rng(4).choice(len(P), 200, replace=False).astype(np.int64)
    got = t.FPFHAt(r, N, ids)
    FO.check(_rows(ref, ids), got[0], got[2], got[3], what="sphere")
    _check_against_full(got, full, P, ids, "sphere")
    assert got[4] == _union(P, ids, r) and got[4] < len(P)


# ------------------------------------------------------------------------------------------------ fat rows

@pytest.mark.parametrize("grid", [None, "2"])
def test_fat_rows(grid, monkeypatch):
    """tests/test_gpu_fpfh.py's heaps of 4095 / 4096 / 4097 and 70 000 coincident records at r = 1: the ids are one
    record inside each heap, background points whose radius reaches one heap and two, and one that reaches none.  All
    three stages meet a set-aside row on the grid (PCGX_GRID=2 keeps it; the library's own choice is the walk)."""
    sc = TF._cached("heaps", TF._heap_scene)
    ref = TF._cached("heaps ref", TF._heap_reference)
    P, N, n_bg, first = sc["points"], sc["normals"], sc["n_bg"], sc["first"]
    sites = np.concatenate([
        n_bg + np.cumsum([0] + TF.HEAP_SIZE[:3]),                    # the first record of each heap (the big one: its site)
        np.nonzero(ref["near_heap"] & ~ref["two_heaps"])[0][:2],     # background, one heap in reach
        np.nonzero(ref["two_heaps"])[0][:2],                         # two heaps
        np.nonzero(~ref["near_heap"])[0][:2]])                       # none
    ids = np.ascontiguousarray(first[sites], np.int64)
    assert len(ids) == 10
    if grid:
        monkeypatch.setenv("PCGX_GRID", grid)
    t = kdtree.New(P)
    if grid:
        _assert_heap_grid(t)
    else:
        assert _grid_on(t)[3] == 0  # no grid: the walk
    what = "heaps, PCGX_GRID=%s" % grid
    full = t.FPFH(TF.R_HEAP, N)
    got = t.FPFHAt(TF.R_HEAP, N, ids)
    f, x, c, m, n_spfh = got
    FO.check(_rows(ref, sites), f, c, m, what=what)
    _check_against_full(got, full, P, ids, what)
    want = _union(P, ids, TF.R_HEAP)
    print(what, "n_spfh", n_spfh, "of", len(P))
    assert n_spfh == want and sum(TF.HEAP_SIZE) < n_spfh < len(P) - 1000, (n_spfh, want)


# ------------------------------------------------------------------------------------------------ the device form

def _dev_call(t, r, dn, ids32, cap, n_ids, sentinel=True, optional=True):
    """FPFHAtDev over ids32 (numpy int32 [cap]) with *d_n_ids = n_ids (None: no count) -> numpy outputs"""
    import torch
    dev = torch.device("cuda", 0)
    di = torch.from_numpy(np.ascontiguousarray(ids32, np.int32)).to(dev)
    dcnt = torch.tensor([0 if n_ids is None else n_ids], dtype=torch.int32, device=dev)
    df = torch.full((cap, 33), 7.5, dtype=torch.float32, device=dev)
    dx = torch.full((cap, 3), 7.5, dtype=torch.float32, device=dev)
    dc = torch.full((cap, 33), -7, dtype=torch.int32, device=dev)
    dm = torch.full((cap,), -7, dtype=torch.int32, device=dev)
    ds = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    t.FPFHAtDev(r, dn.data_ptr(), di.data_ptr(), cap, df.data_ptr(), dx.data_ptr(),
                d_n_ids=0 if n_ids is None else dcnt.data_ptr(), d_counts=dc.data_ptr() if optional else 0,
                d_pairs=dm.data_ptr() if optional else 0, d_n_spfh=ds.data_ptr() if optional else 0, stream=st)
    torch.cuda.synchronize()
    return (df.cpu().numpy(), dx.cpu().numpy(), dc.cpu().numpy().reshape(-1, 3, 11), dm.cpu().numpy(),
            int(ds.cpu().numpy()[0]))


def test_device_form_slots():
    import torch
    sc = _surface()
    P, N, r = sc["P"], sc["N"], sc["r"]
    n, cap = len(P), 128
    t = kdtree.New(P)
    full = t.FPFH(r, N)
    dn = torch.from_numpy(N).to(torch.device("cuda", 0))
    ids = np.random.default_rng(8).choice(n, cap, replace=False).astype(np.int32)
    ids[0], ids[40], ids[99], ids[127] = -1, n, -1, n + 5  # dead ids in live positions
    in_range = (ids >= 0) & (ids < n)
    for n_ids in (-3, 0, 1, 100, 128, 500, None):
        k = cap if n_ids is None else min(max(n_ids, 0), cap)
        live = in_range & (np.arange(cap) < k)
        f, x, c, m, n_spfh = _dev_call(t, r, dn, ids, cap, n_ids)
        what = "n_ids %s" % n_ids
        # every dead slot: zeros in every output (the sentinels are gone: every slot is written)
        assert np.all(_bits(f[~live]) == 0) and np.all(_bits(x[~live]) == 0) and np.all(c[~live] == 0) and np.all(m[~live] == 0), what
        sel = ids[live].astype(np.int64)
        _check_against_full((f[live], x[live], c[live], m[live], n_spfh), full, P, sel, what)
        assert n_spfh == _union(P, sel, r), what
        if n_ids in (100, None):  # the host form's bits (it takes the live ids only: it rejects the others)
            hf, hx, hc, hm, hs = t.FPFHAt(r, N, sel)
            assert np.array_equal(_bits(hf), _bits(f[live])) and np.array_equal(hc, c[live]) and hs == n_spfh, what
    # without the optional outputs
    f2, x2, _, _, _ = _dev_call(t, r, dn, ids, cap, 100, optional=False)
    f1, x1, _, _, _ = _dev_call(t, r, dn, ids, cap, 100)
    assert np.array_equal(_bits(f1), _bits(f2)) and np.array_equal(_bits(x1), _bits(x2))
    # cap == 0: PCGX_OK, nothing written but the record count
    ds = torch.full((1,), -7, dtype=torch.int32, device=dn.device)
    t.FPFHAtDev(r, dn.data_ptr(), 0, 0, 0, 0, d_n_spfh=ds.data_ptr())
    torch.cuda.synchronize()
    assert int(ds.cpu()[0]) == 0
    t.FPFHAtDev(r, dn.data_ptr(), 0, 0, 0, 0)


def test_flags_do_not_leak_between_calls_and_calls_repeat():
    """Large id set, then a small one on the same handle (the arena hands the second call the first call's flags and
    records back): each result is a fresh handle's, and two identical calls give the same bits."""
    sc = _surface()
    P, N, r = sc["P"], sc["N"], sc["r"]
    rng = np.random.default_rng(21)
    big = rng.choice(len(P), 1500, replace=False).astype(np.int64)
    small = rng.choice(len(P), 3, replace=False).astype(np.int64)
    t = kdtree.New(P)
    a_big, a_small, a_small2 = t.FPFHAt(r, N, big), t.FPFHAt(r, N, small), t.FPFHAt(r, N, small)
    b_small = kdtree.New(P).FPFHAt(r, N, small)
    b_big = kdtree.New(P).FPFHAt(r, N, big)
    for a, b in ((a_big, b_big), (a_small, b_small), (a_small, a_small2)):
        for u, v in zip(a[:4], b[:4]):
            assert np.array_equal(_bits(u), _bits(v))
        assert a[4] == b[4]
    assert a_small[4] == _union(P, small, r) and a_small[4] < a_big[4] <= len(P)


def test_bad_arguments():
    P, N, r = TF._scene("cube")
    t = kdtree.New(P)
    lib = L.lib()
    ids = np.arange(5, dtype=np.int64)
    out = np.empty((5, 33), f32)
    p16 = C.c_void_p(16)

    def host(h=t._h, nrm=L.ptr(N), radius=r, i=L.ptr(ids), k=5, f=L.ptr(out)):
        return lib.pcgx_kdtree_fpfh_at(h, nrm, radius, i, k, f, None, None, None, None)

    def devf(h=t._h, nrm=p16, radius=r, i=p16, k=5, f=p16):
        return lib.pcgx_kdtree_fpfh_at_dev(h, nrm, radius, i, k, None, f, None, None, None, None, None)

    assert host() == L.PCGX_OK
    for call in (host, devf):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert call(radius=bad) == L.PCGX_E_INVALID
        assert call(h=None) == L.PCGX_E_INVALID
        assert call(nrm=None) == L.PCGX_E_INVALID
        assert call(i=None) == L.PCGX_E_INVALID   # NULL ids with a positive count
        assert call(f=None) == L.PCGX_E_INVALID   # NULL fpfh with a positive count
        assert call(k=-1) == L.PCGX_E_INVALID     # a negative count
        assert call(k=0, i=None, f=None) == L.PCGX_OK
    # the host form can read the list: an id out of range is an error
    for bad in (-1, len(P)):
        ids2 = ids.copy()
        ids2[3] = bad
        assert host(i=L.ptr(ids2)) == L.PCGX_E_INVALID
    with pytest.raises(ValueError):
        t.FPFHAt(r, N[:-1], ids)
    f, x, c, m, n_spfh = t.FPFHAt(r, N, np.zeros(0, np.int64))
    assert f.shape == (0, 33) and x.shape == (0, 3) and n_spfh == 0


# ------------------------------------------------------------------------------------------------ the chain

def test_chain_with_no_read_back():
    """NormalsDev, ISSKeypointsDev and FPFHAtDev(cap) on both moved clouds, CorrespondencesDev over the two padded
    descriptor arrays (na = nb = cap: the padding is zero rows) and EstimatePoseDev over the two compact xyz arrays, on
    one stream with nothing read back before the final synchronise.  The pose's bits are those of the same chain over
    the full FPFHDev and a torch gather at ids[:n] (the descriptor rows are the full call's bit for bit)."""
    import torch
    P, P2 = PO.moved_clouds()
    r, vp, vp2 = 0.1, (0.8, 0.8, 50.0), (-0.8 + 2.25, 0.8 - 0.5, 50.0 + 1.75)
    t, t2 = kdtree.New(P), kdtree.New(P2)
    n, n_hyp, max_dist = len(P), 2048, 0.01
    cap = 1 << (int(n // 16).bit_length() - 1)  # the power of two at or below Len() / 16
    assert cap == 128
    dev = torch.device("cuda", 0)
    samples = alignment.Samples(n_hyp, 3)

    def buf(shape, dtype=torch.float32, fill=None):
        return torch.empty(shape, dtype=dtype, device=dev) if fill is None else torch.full(shape, fill, dtype=dtype, device=dev)

    du = torch.from_numpy(samples.view(np.int32)).to(dev)
    dn, dn2 = buf((n, 3)), buf((n, 3))
    dk, dk2, counts = buf(n, torch.int32), buf(n, torch.int32), buf((2,), torch.int32, -1)
    fa, fb, xa, xb = buf((cap, 33), fill=7.5), buf((cap, 33), fill=7.5), buf((cap, 3), fill=7.5), buf((cap, 3), fill=7.5)
    spfh = buf((2,), torch.int32, -1)
    src, dst, cnt = buf(cap, torch.int32), buf(cap, torch.int32), buf(1, torch.int32)
    res = buf(alignment.RESULT_WORDS, torch.int32)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        for tree, view, nrm, keys, k, f, x in ((t, vp, dn, dk, 0, fa, xa), (t2, vp2, dn2, dk2, 1, fb, xb)):
            tree.NormalsDev(r, nrm.data_ptr(), Viewpoint=view, stream=st)
            tree.ISSKeypointsDev(0.15, 0.1, keys.data_ptr(), counts.data_ptr() + 4 * k, stream=st)
            tree.FPFHAtDev(r, nrm.data_ptr(), keys.data_ptr(), cap, f.data_ptr(), x.data_ptr(),
                           d_n_ids=counts.data_ptr() + 4 * k, d_n_spfh=spfh.data_ptr() + 4 * k, stream=st)
        features.CorrespondencesDev(fa.data_ptr(), cap, fb.data_ptr(), cap, src.data_ptr(), dst.data_ptr(), cnt.data_ptr(),
                                    MaxRatio=1.0, Mutual=True, stream=st)
        alignment.EstimatePoseDev(xa.data_ptr(), cap, xb.data_ptr(), cap, src.data_ptr(), dst.data_ptr(), cap, du.data_ptr(),
                                  n_hyp, res.data_ptr(), max_dist, d_n_pairs=cnt.data_ptr(), stream=st)
        stream.synchronize()  # the first wait, and nothing was read before it
    torch.cuda.synchronize()
    na, nb = (int(v) for v in counts.cpu().numpy())
    got = alignment.ReadResult(res.cpu().numpy())
    print("keypoints: %d and %d of cap %d, SPFH records: %s of %d, pairs: %d, inliers: %d"
          % (na, nb, cap, spfh.cpu().numpy().tolist(), n, int(cnt.cpu().numpy()[0]), got["n_inliers"]))
    assert 30 < na <= cap and 30 < nb <= cap
    assert np.all(spfh.cpu().numpy() < n)
    assert np.all(fa[na:].cpu().numpy() == 0) and np.all(xb[nb:].cpu().numpy() == 0)
    assert got["found"]
    assert np.max(np.linalg.norm(mat.Transform(got["pose"], P).astype(f64) - P2, axis=1)) < max_dist

    # the parent's chain over the same keypoints: the full FPFHDev, one read of the counts, torch gathers
    dP, dP2 = torch.from_numpy(P).to(dev), torch.from_numpy(P2).to(dev)
    df, df2 = buf((n, 33)), buf((n, 33))
    res2 = buf(alignment.RESULT_WORDS, torch.int32)
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        t.FPFHDev(r, dn.data_ptr(), df.data_ptr(), stream=st)
        t2.FPFHDev(r, dn2.data_ptr(), df2.data_ptr(), stream=st)
        ka, kb = dk[:na].long(), dk2[:nb].long()
        ga, gb = df[ka].contiguous(), df2[kb].contiguous()
        pa, pb = dP[ka].contiguous(), dP2[kb].contiguous()
        src2, dst2, cnt2 = buf(na, torch.int32), buf(na, torch.int32), buf(1, torch.int32)
        features.CorrespondencesDev(ga.data_ptr(), na, gb.data_ptr(), nb, src2.data_ptr(), dst2.data_ptr(), cnt2.data_ptr(),
                                    MaxRatio=1.0, Mutual=True, stream=st)
        alignment.EstimatePoseDev(pa.data_ptr(), na, pb.data_ptr(), nb, src2.data_ptr(), dst2.data_ptr(), na, du.data_ptr(),
                                  n_hyp, res2.data_ptr(), max_dist, d_n_pairs=cnt2.data_ptr(), stream=st)
        stream.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(fa[:na].cpu().numpy()), _bits(ga.cpu().numpy()))
    assert np.array_equal(_bits(xa[:na].cpu().numpy()), _bits(pa.cpu().numpy()))
    m = int(cnt.cpu().numpy()[0])
    assert m == int(cnt2.cpu().numpy()[0])
    assert np.array_equal(src[:m].cpu().numpy(), src2[:m].cpu().numpy()) and np.array_equal(dst[:m].cpu().numpy(), dst2[:m].cpu().numpy())
    want = alignment.ReadResult(res2.cpu().numpy())
    assert want["found"] and np.array_equal(_bits(got["pose"]), _bits(want["pose"]))
    assert got["n_inliers"] == want["n_inliers"]
