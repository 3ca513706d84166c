"""csrc/m3c2_terms.h compiled for the host with g++ -ffp-contract=off (tests/cpp/m3c2_terms_host.cpp over the shim
tests/cpp/host_shim): the member test and the finish that the kernels compile give the NumPy oracle's answers
(tests/m3c2_oracle.py) by array_equal, on random and edge inputs; and the range superset, which is a condition and not a
tolerance: every member's a lies in [a_lo, a_hi] and in the clipped range, has exactly one owning slab, and is reported by
that slab's float32 ball under ray_bound -- over 120 000 (core, axis, point) triples at coordinates up to 4096 and axis
lengths from 1e-3 to 1e3."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import m3c2_oracle as MO  # noqa: E402
import m3c2_scenes as MS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
nan, inf = np.nan, np.inf


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("m3c2_terms") / "libm3c2_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "m3c2_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _c(a):
    return np.ascontiguousarray(a, f32).reshape(-1, 3)


def member_pairs(lib, o, d, rho, half, p):
    o, d, p = _c(o), _c(d), _c(p)
    m = len(o)
    us, mem = np.full(m, -1, np.int32), np.full(m, -1, np.int32)
    a, cc, lo, hi = (np.zeros(m, f64) for _ in range(4))
    lib.cyl_member_batch(_p(o), _p(d), ctypes.c_float(rho), ctypes.c_float(half), _p(p), ctypes.c_int64(m), _p(us), _p(mem),
                         _p(a), _p(cc), _p(lo), _p(hi))
    return us, mem, a, cc, lo, hi


def _check_pairs(lib, o, d, rho, half, p):
    us, mem, a, cc, lo, hi = member_pairs(lib, o, d, rho, half, p)
    o, d, p = _c(o), _c(d), _c(p)
    dd, rrdd, lldd, usable = MO.cyl_terms(o, d, rho, half)
    assert np.array_equal(us, usable.astype(np.int32))
    with np.errstate(all="ignore"):
        want_hi = np.sqrt(lldd) * (1.0 + 2.0 ** -50)
    assert np.array_equal(hi, want_hi, equal_nan=True) and np.array_equal(lo, -want_hi, equal_nan=True)
    for f in range(0, len(o), 256):  # the oracle makes all pairs of a block: its diagonal
        e = min(f + 256, len(o))
        m, wa = MO.members(p[f:e], o[f:e], d[f:e], rho, half)
        k = np.arange(e - f)
        assert np.array_equal(mem[f:e], m[k, k].astype(np.int32))
        assert np.array_equal(a[f:e], wa[k, k], equal_nan=True)
    return mem, a, lo, hi


def _near_axes(rng, o, d, rho, half, reach=1.5):
    """One point near each cylinder: on the axis within reach * half (metric) of the core, pushed sideways by
    0 .. reach * rho."""
    o64, d64 = o.astype(f64), d.astype(f64)
    unit = d64 / np.linalg.norm(d64, axis=1, keepdims=True)
    side = np.cross(unit, rng.normal(size=(len(o), 3)))
    side /= np.maximum(np.linalg.norm(side, axis=1, keepdims=True), 1e-300)
    along = rng.uniform(-reach, reach, (len(o), 1)) * half
    return (o64 + along * unit + side * (rng.uniform(0.0, reach, (len(o), 1)) * rho)).astype(f32)


def test_member_test_matches_the_oracle_on_random_pairs(host):
    rng = np.random.default_rng(31)
    m = 6000
    o = rng.uniform(-10, 10, (m, 3)).astype(f32)
    d = (rng.normal(size=(m, 3)) * 10.0 ** rng.uniform(-3, 3, (m, 1))).astype(f32)
    rho, half = 0.25, 1.5
    p = _near_axes(rng, o, d, rho, half)
    mem = _check_pairs(host, o, d, rho, half, p)[0]
    assert 0.2 * m < mem.sum() < 0.8 * m  # both answers are exercised


def test_member_test_on_edge_inputs(host):
    o = np.zeros((12, 3), f32)
    d = np.tile(f32([1, 0, 0]), (12, 1))
    p = np.tile(f32([0.5, 0, 0]), (12, 1))
    o[0, 1] = nan            # NaN core
    o[1, 0] = inf            # infinite core
    d[2] = 0                 # dd == 0
    d[3] = [0, -0.0, 0]      # ... with a negative zero
    d[4, 2] = nan
    d[5, 0] = -inf
    p[6, 1] = nan            # a NaN point
    p[7, 0] = inf            # an infinite point on the axis
    p[8] = [-0.5, 0, 0]      # behind the core: the cylinder runs both ways
    d[9] = [1e-30, 0, 0]     # a tiny axis: dd = 1e-60 is no underflow in float64
    d[10] = [0, 3e18, 0]     # a huge one
    p[10] = [0, -0.5, 0]
    d[11] = [-2, 0, 0]       # reversed: the same cylinder
    mem = _check_pairs(host, o, d, 0.25, 1.0, p)[0]
    assert list(mem) == [0] * 8 + [1, 1, 1, 1]


def test_side_surface_and_caps_are_inclusive(host):
    """tests/m3c2_scenes.py's dyadic points, every product exact: rho = 0.5, L = 2; a point at offset exactly 0.5 or at
    exactly +-2 along the axis is a member, the next float32 outside is not."""
    p, member = MS.dyadic()
    o = np.zeros_like(p)
    for axis in MS.DYADIC_AXES:  # the metric size does not depend on |axis|
        mem = _check_pairs(host, o, np.tile(f32(axis), (len(p), 1)), MS.DYADIC_RHO, MS.DYADIC_HALF, p)[0]
        assert np.array_equal(mem, member.astype(np.int32)) and 0 < member.sum() < len(p), axis


def cover(lib, o, d, rho, half, lo, hi, target, p):
    o, d, p = _c(o), _c(d), _c(p)
    lo, hi = np.ascontiguousarray(lo, f32), np.ascontiguousarray(hi, f32)
    out, ks = np.zeros(5, np.int64), ctypes.c_int32()
    lib.cyl_cover_check(_p(o), _p(d), ctypes.c_float(rho), ctypes.c_float(half), _p(lo), _p(hi), ctypes.c_float(target),
                        _p(p), ctypes.c_int64(len(o)), _p(out), ctypes.byref(ks))
    names = ("members", "outside_range", "not_one_owner", "ball_missed", "too_many_slabs")
    return dict(zip(names, map(int, out))), ks.value


@pytest.mark.parametrize("shift,extent,rho,half", [(0.0, 10.0, 0.05, 0.5), (0.0, 10.0, 0.05, 4.0),
                                                   (4090.0, 6.0, 2.0 ** -6, 0.25), (-4096.0, 8.0, 0.1, 0.1),
                                                   (0.0, 4096.0, 1.0, 300.0)])
def test_range_superset_and_cover(host, shift, extent, rho, half):
    """24 000 triples per scene and slab length, five scenes, two lengths: |coordinate| <= 4096, |axis| 1e-3 .. 1e3."""
    rng = np.random.default_rng(int(abs(shift)) + int(100 * half) + 7)
    m = 24_000
    o = (shift + rng.uniform(0, extent, (m, 3))).astype(f32)
    d = (rng.normal(size=(m, 3)) * 10.0 ** rng.uniform(-3, 3, (m, 1))).astype(f32)
    p = _near_axes(rng, o, d, rho, half, reach=1.05)  # most of them members, many near the caps and the side
    p[::4] = (o.astype(f64) + (d.astype(f64) / np.linalg.norm(d.astype(f64), axis=1, keepdims=True) *
                               rng.choice([-1.0, 1.0], (m, 1)) * half))[::4].astype(f32)  # on a cap's centre, up to rounding
    lo = np.minimum(p.min(0), o.min(0))  # the box holds the points (and may hold more)
    hi = np.maximum(p.max(0), o.max(0))
    assert max(np.abs(lo).max(), np.abs(hi).max()) <= 4096 + 2 * half + 1
    for target in (2 * rho, 7.3 * rho):  # a walk's slab length, and a grid cell's
        out, ks = cover(host, o, d, rho, half, lo, hi, target, p)
        assert out["members"] > 0.5 * m, out
        assert out["outside_range"] == 0 and out["not_one_owner"] == 0 and out["ball_missed"] == 0, out
        assert out["too_many_slabs"] == 0, (out, ks)
        assert ks >= min(2, int(2 * half / target))


def finish(lib, axes, n1, s1, n2, s2, reg, k):
    axes = _c(axes)
    m = len(axes)
    n1, n2 = np.ascontiguousarray(n1, np.int32), np.ascontiguousarray(n2, np.int32)
    s1, s2 = np.ascontiguousarray(s1, f64), np.ascontiguousarray(s2, f64)
    dist, lod, sig = np.full(m, 7.0), np.full(m, 7.0), np.full(m, 7, np.uint8)
    lib.m3c2_finish_batch(_p(axes), _p(n1), _p(s1), _p(n2), _p(s2), ctypes.c_int64(m), ctypes.c_double(reg),
                          ctypes.c_int32(k), _p(dist), _p(lod), _p(sig))
    return dist, lod, sig


def _same(got, want):
    return all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))


def test_finish_matches_numpy(host):
    rng = np.random.default_rng(4)
    m = 20_000
    axes = (rng.normal(size=(m, 3)) * 10.0 ** rng.uniform(-3, 3, (m, 1))).astype(f32)
    axes[::211] = 0
    axes[5::211, 1] = nan
    axes[9::211, 2] = inf
    n1, n2 = rng.integers(0, 60, m).astype(np.int32), rng.integers(0, 60, m).astype(np.int32)
    dd = (axes.astype(f64) ** 2).sum(1)

    def sums(n, shift):  # what cylinders along these axes would hold: a = s dd, s about shift +- 0.1
        with np.errstate(all="ignore"):
            mean = (shift + rng.normal(scale=0.05, size=m)) * dd
            s1 = mean * n
            s2 = (mean * mean + (0.1 * dd) ** 2 * rng.uniform(0, 1, m)) * n
        s2[::3] = (s1 * s1 / np.maximum(n, 1))[::3] * (1 - 1e-15)  # a variance that comes out below 0
        return np.stack([s1, s2], axis=1)
    s1, s2 = sums(n1, 0.0), sums(n2, rng.choice([0.0, 0.01, 0.3], m))
    for reg, k in ((0.0, 2), (0.02, 4), (2.0 ** -6, 10)):
        n1k = n1.copy()
        n1k[::5] = k - 1  # one short of min_count
        n1k[1::5] = k
        got = finish(host, axes, n1k, s1, n2, s2, reg, k)
        want = MO.finish(axes, n1k, s1, n2, s2, reg, k)
        assert _same(got, want), (reg, k)
        ok = ~np.isnan(got[0])
        assert np.isnan(got[0][::5]).all() and np.isnan(got[1][::5]).all() and not got[2][::5].any()
        assert ok.sum() > 0.3 * m and got[2][ok].any() and not got[2][ok].all()
        assert np.array_equal(np.isnan(got[0]), np.isnan(got[1])) and not got[2][~ok].any()


def test_finish_on_tiny_and_huge_axes(host):
    axes = f32([[1e-20, 0, 0], [0, 3e18, 0], [0, 0, 1], [2.0 ** -70, 0, 0], [2.0 ** 60, 0, 0]])
    dd = (axes.astype(f64) ** 2).sum(1)
    n = np.full(5, 4, np.int32)
    a1 = np.array([0.0, 0.25, 0.5, 0.75])[None, :] * dd[:, None]  # a = s dd at s = 0 .. 0.75
    a2 = a1 + 0.5 * dd[:, None]
    s1 = np.stack([a1.sum(1), (a1 * a1).sum(1)], axis=1)
    s2 = np.stack([a2.sum(1), (a2 * a2).sum(1)], axis=1)
    got = finish(host, axes, n, s1, n, s2, 0.0, 4)
    assert _same(got, MO.finish(axes, n, s1, n, s2, 0.0, 4))
    norm = np.sqrt(dd)
    assert np.allclose(got[0], 0.5 * norm, rtol=1e-14, atol=0) and np.all(np.isfinite(got[1]))
    # a variance clipped at 0: four equal terms whose S2 came out below S1 S1 / n
    s = np.array([[4 * 0.1, 4 * 0.1 * 0.1 * (1 - 1e-12)]])
    got = finish(host, f32([[0, 0, 1]]), [4], s, [4], s, 0.25, 2)
    assert got[0][0] == 0.0 and got[1][0] == 1.96 * 0.25 and got[2][0] == 0
