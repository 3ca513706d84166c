"""csrc/shape_terms.h compiled for the host with g++ -ffp-contract=off (tests/cpp/shape_terms_host.cpp over the shim
tests/cpp/host_shim): the status, the record, the partner rule's mix, the inlier test and the refit the kernels of
shapes.hip compile give the NumPy oracle's bits (tests/shape_oracle.py) on random oriented pairs at four scales,
near-parallel normals, +-0, denormals, NaN and infinities, axes with tied largest components, and 10^4 (word, id) pairs."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shape_oracle as SO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, u32 = np.float32, np.float64, np.uint32
KINDS = (SO.SPHERE, SO.CYLINDER)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shape_terms") / "libshape_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "shape_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(u32 if a.dtype == f32 else np.uint64)


def check_hypotheses(lib, kind, pairs, has=None, axis=None, cos=0.0, r_min=0.0, r_max=np.inf):
    pairs = np.ascontiguousarray(pairs, f32).reshape(-1, 4, 3)
    m = len(pairs)
    has = np.ascontiguousarray(has if has is not None else np.ones(m), np.int32)
    ax = np.ascontiguousarray(axis, f32) if axis is not None else None
    st, rec = np.full(m, -9, np.int32), np.full((m, 8), 7, f32)
    lib.shape_hypothesis_batch(kind, _p(pairs), _p(has), ctypes.c_int64(m), _p(ax), ctypes.c_float(cos),
                               ctypes.c_float(r_min), ctypes.c_float(r_max), _p(st), _p(rec))
    A = SO.Axis(axis, cos) if axis is not None else None
    for k, q in enumerate(pairs):
        ws, wr = SO.hypothesis(kind, bool(has[k]), q[0], q[1], q[2], q[3], A, r_min, r_max)
        assert st[k] == ws, (k, q, st[k], ws)
        assert np.array_equal(bits(rec[k]), bits(wr)), (k, q, rec[k], wr)
    return st, rec


def random_pairs(rng, m, scale):
    """points near a sphere of radius about scale, with roughly radial normals of any length"""
    d = rng.standard_normal((m, 2, 3))
    d /= np.linalg.norm(d, axis=2)[:, :, None]
    c = rng.standard_normal((m, 1, 3)) * scale * 3
    p = c + d * scale * (1 + 0.05 * rng.standard_normal((m, 2, 1)))
    nrm = (d + 0.1 * rng.standard_normal((m, 2, 3))) * rng.uniform(0.2, 3, (m, 2, 1))
    return np.stack([p[:, 0], nrm[:, 0], p[:, 1], nrm[:, 1]], axis=1).astype(f32)


def test_codes(host):
    out = (ctypes.c_int32 * 8)()
    host.shape_codes(out)
    assert list(out) == [SO.NOT_RUN, SO.OK, SO.NO_PARTNER, SO.DEGENERATE, SO.AXIS, SO.RADIUS, SO.SPHERE, SO.CYLINDER]
    assert list(out) == [-1, 0, 1, 2, 3, 4, 0, 1]


@pytest.mark.parametrize("kind", KINDS)
def test_random_oriented_pairs(host, kind):
    rng = np.random.default_rng(5 + kind)
    pairs = np.concatenate([random_pairs(rng, 250, s) for s in (1e-3, 1.0, 50.0, 1e6)])
    st, rec = check_hypotheses(host, kind, pairs)
    assert (st == SO.OK).sum() > 900
    if kind == SO.CYLINDER:
        a = rec[st == SO.OK, 4:7].astype(f64)
        assert np.all(np.abs(np.linalg.norm(a, axis=1) - 1) < 1e-6)
        assert np.all(np.take_along_axis(a, np.abs(a).argmax(axis=1)[:, None], 1) > 0)
        assert np.all(np.abs(np.einsum("ij,ij->i", rec[st == SO.OK, :3].astype(f64), a)) < 1e-4 * (1 + np.abs(rec[st == SO.OK, :3]).max(axis=1)))
    for axis, cos in (((0, 0, 1), 0.0), ((0, 0, 1), 0.9), ((1, -2, 0.5), 0.5), ((-3, 0, 0), 0.2)):
        st, rec = check_hypotheses(host, kind, pairs[250:650], axis=axis, cos=cos)
        assert (st == SO.OK).any() and (kind == SO.SPHERE or cos == 0.0 or (st == SO.AXIS).any())
        if kind == SO.CYLINDER:
            assert np.all(rec[st == SO.OK, 4:7].astype(f64) @ np.asarray(axis, f64) >= 0)
    # a radius window that cuts the middle out of the scale-1 pairs, and a seed without a partner
    st, _ = check_hypotheses(host, kind, pairs[250:500], r_min=0.9, r_max=1.1)
    assert (st == SO.RADIUS).any() and (st == SO.OK).any()
    has = np.ones(250, np.int32)
    has[::3] = 0
    st, rec = check_hypotheses(host, kind, pairs[250:500], has=has)
    assert np.all(st[::3] == SO.NO_PARTNER) and np.all(rec[::3] == 0)


@pytest.mark.parametrize("kind", KINDS)
def test_near_parallel_zero_denormal_and_non_finite(host, kind):
    rng = np.random.default_rng(9)
    base = random_pairs(rng, 40, 1.0)
    near = base.copy()
    for k, eps in enumerate(np.logspace(-9, -3, 40)):  # the angle between the normals across the 1e-12 bound
        near[k, 3] = near[k, 1] * f32(1.5) + f32(eps) * np.array([near[k, 1, 1], -near[k, 1, 0], 0], f32)
    st, _ = check_hypotheses(host, kind, near)
    assert (st == SO.DEGENERATE).any() and (st != SO.DEGENERATE).any()
    par = base.copy()
    par[:, 3] = -par[:, 1]  # exactly parallel
    st, _ = check_hypotheses(host, kind, par)
    assert np.all(st == SO.DEGENERATE)
    odd = [0.0, -0.0, 1e-45, -1e-45, 1e-39, 3e38, -3e38, np.nan, np.inf, -np.inf, 1.0, -1.0]
    cases = []
    for v in odd:
        for slot in range(12):
            q = base[slot % 40].copy().reshape(-1)
            q[slot] = v
            cases.append(q)
        cases.append(np.full(12, v, f32))
    check_hypotheses(host, kind, np.array(cases, f32))
    tiny = (base * f32(1e-41)).astype(f32)
    check_hypotheses(host, kind, tiny)
    # the same point twice with crossing normals: the lines meet in it, the radius is 0
    same = base.copy()
    same[:, 2] = same[:, 0]
    st, rec = check_hypotheses(host, kind, same)
    assert np.all(rec[st == SO.OK, 3] < 1e-5)
    st, _ = check_hypotheses(host, kind, same, r_min=1e-3)
    assert np.all((st == SO.RADIUS) | (st == SO.DEGENERATE))


def test_tied_orient_components_and_the_axis_at_equality(host):
    # normals whose cross product has tied largest components: n0 x n1 for unit vectors of the coordinate planes
    cases = []
    for n0, n1 in (((1, 0, 0), (0, 1, 1)), ((1, 0, 0), (0, -1, 1)), ((0, 1, 0), (1, 0, -1)), ((1, 1, 0), (0, 0, 1)),
                   ((1, -1, 0), (0, 0, -1)), ((1, 1, 0), (1, -1, 0)), ((0, 1, 1), (0, 1, -1))):
        cases.append(np.array([(1, 2, 3), n0, (2, 1, 1), n1], f32))
    pairs = np.array(cases, f32)
    st, rec = check_hypotheses(host, SO.CYLINDER, pairs)
    assert np.all(st == SO.OK)
    a = rec[:, 4:7]
    assert np.all(np.take_along_axis(a, np.abs(a).argmax(axis=1)[:, None], 1) > 0)
    # the axis test at equality: a = z exactly, the axis (3, 0, 4): |a . axis| = 4 = 0.8 * 5; (0, 0, 1) with a = z: 1 = 1
    up = np.array([[(1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 1, 0)]], f32)
    for cos, want in ((0.8, None), (float(np.nextafter(f32(0.8), f32(1))), SO.AXIS), (float(np.nextafter(f32(0.8), f32(0))), SO.OK)):
        st, rec = check_hypotheses(host, SO.CYLINDER, up, axis=(3, 0, 4), cos=cos)
        # (float32 0.8 is above 0.8: 0.8f * 5 > 4, so the bound at "equality" is the float32's own)
        assert want is None or st[0] == want
    st, rec = check_hypotheses(host, SO.CYLINDER, up, axis=(0, 0, 1), cos=1.0)
    assert st[0] == SO.OK and rec[0].tolist() == [0, 0, 0, 1, 0, 0, 1, 0]
    st, rec = check_hypotheses(host, SO.CYLINDER, up, axis=(0, 0, -2), cos=1.0)
    assert st[0] == SO.OK and rec[0].tolist() == [0, 0, 0, 1, 0, 0, -1, 0]
    st, _ = check_hypotheses(host, SO.CYLINDER, up, axis=(1, 0, 0), cos=0.0)
    assert st[0] == SO.OK  # perpendicular, the bound 0: |a . axis| = 0 >= 0


def test_mix_and_key(host):
    rng = np.random.default_rng(3)
    m = 10000
    u1 = rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(u32)
    ids = rng.integers(0, 2 ** 31 - 1, m, dtype=np.int64).astype(u32)
    u1[:4], ids[:4] = (0, 0xffffffff, 0, 0xffffffff), (0, 0, 0x7ffffffe, 0x7ffffffe)
    x, key = np.zeros(m, u32), np.zeros(m, np.uint64)
    host.shape_mix_batch(_p(u1), _p(ids), ctypes.c_int64(m), _p(x), _p(key))
    want = np.array([SO.mix(u, [i])[0] for u, i in zip(u1[:200], ids[:200])], u32)
    assert np.array_equal(x[:200], want)
    for u in (0, 12345, 0xffffffff):  # one word, many ids: the vector form
        xv = np.zeros(m, u32)
        host.shape_mix_batch(_p(np.full(m, u, u32)), _p(ids), ctypes.c_int64(m), _p(xv), _p(key))
        assert np.array_equal(xv, SO.mix(u, ids))
        assert np.array_equal(key, (xv.astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64))
        assert SO.partner(u, ids.astype(np.int64)) == int(ids[np.argmin(key)])
    # the reference values of the finaliser (MurmurHash3's fmix32) on id 0: x = fmix32(u1)
    assert int(SO.mix(1, [0])[0]) == 0x514E28B7 and int(SO.mix(0, [0])[0]) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_inlier_test(host, kind):
    rng = np.random.default_rng(11 + kind)
    for scale, md in ((1.0, 0.02), (1e-3, 1e-4), (200.0, 0.5)):
        rec = np.zeros(8, f32)
        rec[:3] = rng.standard_normal(3) * scale
        rec[3] = scale
        a = rng.standard_normal(3)
        if kind == SO.CYLINDER:
            rec[4:7] = a / np.linalg.norm(a)
        d = rng.standard_normal((4000, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        P = (rec[:3] + d * scale * (1 + rng.uniform(-3, 3, (4000, 1)) * md / scale)).astype(f32)
        if kind == SO.CYLINDER:
            P = (P + rng.uniform(-2, 2, (4000, 1)) * scale * rec[4:7]).astype(f32)
        M = (d + 0.4 * rng.standard_normal((4000, 3))).astype(f32)
        P[::97, 1] = np.nan
        M[5::97, 2] = np.nan
        for cos in (0.0, 0.8, 1.0):
            for r in (rec[3], f32(md / 2), f32(md)):  # lo > 0, lo < 0, lo == 0
                q = rec.copy()
                q[3] = r
                got = np.full(4000, -1, np.int32)
                host.shape_inlier_batch(kind, _p(q), _p(P), _p(M), ctypes.c_int64(4000), ctypes.c_float(md), ctypes.c_float(cos),
                                        _p(got))
                want = SO.inlier_mask(kind, q, P, md, M, cos)
                assert np.array_equal(got, want.astype(np.int32)), (scale, cos, r)
                assert not want[::97].any() and (cos == 0.0 or not want[5::97].any())
        assert 0 < SO.inlier_mask(kind, rec, P, md, M, 0.0).sum() < 4000
    r = np.array([1.0, 0.02, 0.01, 0.0, 1e-45, np.nan, np.inf, 3e38], f32)
    lo2, hi2 = np.zeros(8, f32), np.zeros(8, f32)
    host.shape_band_batch(_p(r), ctypes.c_int64(8), ctypes.c_float(0.02), _p(lo2), _p(hi2))
    want = [SO.band(v, 0.02) for v in r]
    assert np.array_equal(bits(lo2), bits(np.array([w[0] for w in want], f32)))
    assert np.array_equal(bits(hi2), bits(np.array([w[1] for w in want], f32)))
    assert lo2[1] == -1 and lo2[2] == -1 and lo2[0] > 0


@pytest.mark.parametrize("kind", KINDS)
def test_refit_terms_and_solve(host, kind):
    rng = np.random.default_rng(21 + kind)
    recs, ns, sums = [], [], []
    for scale in (1e-2, 1.0, 30.0):
        for case in range(8):
            rec = np.zeros(8, f32)
            rec[:3] = rng.standard_normal(3) * scale * 2
            rec[3] = scale
            a = rng.standard_normal(3)
            a[case % 3] = 0 if case < 3 else a[case % 3]
            if case == 6:
                a = np.array([1.0, 1.0, 1.0])  # tied smallest components: the first wins
            if kind == SO.CYLINDER:
                rec[4:7] = a / np.linalg.norm(a)
            m = (5, 40, 700)[case % 3]
            d = rng.standard_normal((m, 3))
            if case == 7:
                d[:] = d[0]  # every point the same: no refit
            d /= np.linalg.norm(d, axis=1)[:, None]
            off = rng.standard_normal(3) * 0.05 * scale
            P = (rec[:3] + off + d * scale * 1.1).astype(f32)
            x, terms = np.zeros((m, 3), f64), np.zeros((m, 13), f64)
            host.shape_refit_terms_batch(kind, _p(rec), _p(P), ctypes.c_int64(m), _p(x), _p(terms))
            want = SO.refit_coords(kind, rec, P)
            assert np.array_equal(bits(x), bits(want)), (scale, case)
            q = (want[:, 0] * want[:, 0] + want[:, 1] * want[:, 1]) + want[:, 2] * want[:, 2]
            assert np.array_equal(bits(terms[:, 12]), bits(q)) and np.array_equal(bits(terms[:, 9]), bits(q * want[:, 0]))
            assert np.array_equal(bits(terms[:, 4]), bits(want[:, 0] * want[:, 1]))
            recs.append(rec)
            ns.append(float(m))
            sums.append(SO.refit_sums(want))
    recs, ns, sums = np.array(recs, f32), np.array(ns, f64), np.array(sums, f64)
    for r_min, r_max in ((0.0, np.inf), (0.5, 2.0)):
        ok, out = np.full(len(ns), -1, np.int32), np.full((len(ns), 8), 7, f32)
        host.shape_refit_batch(kind, _p(recs), _p(ns), _p(sums), ctypes.c_int64(len(ns)), ctypes.c_float(r_min),
                               ctypes.c_float(r_max), _p(ok), _p(out))
        for k in range(len(ns)):
            wok, wrec = SO.refit_from_sums(kind, recs[k], ns[k], sums[k], r_min, r_max)
            assert bool(ok[k]) == wok and np.array_equal(bits(out[k]), bits(wrec)), (k, out[k], wrec)
        assert ok.any() and not ok.all()
    # non-finite and empty sums: no refit, a zero record
    bad = np.array([np.full(13, np.nan), np.full(13, np.inf), np.zeros(13)], f64)
    ok, out = np.full(3, -1, np.int32), np.full((3, 8), 7, f32)
    host.shape_refit_batch(kind, _p(recs[:3].copy()), _p(np.array([4.0, 4.0, 0.0])), _p(bad), ctypes.c_int64(3),
                           ctypes.c_float(0), ctypes.c_float(np.inf), _p(ok), _p(out))
    assert not ok.any() and np.all(out == 0)
    for k in range(3):
        assert not SO.refit_from_sums(kind, recs[k], (4.0, 4.0, 0.0)[k], bad[k])[0]
