"""csrc/ray_terms.h compiled for the host with g++ -ffp-contract=off (tests/cpp/ray_terms_host.cpp over the shim
tests/cpp/host_shim): the member test, the comparison and the box clip that the kernel compiles give the NumPy oracle's
answers (tests/rays_oracle.py) by array_equal, on random and adversarial inputs; and the cover property, which is a
condition and not a tolerance: every member lies in the clipped range, has exactly one owning slab, and is reported by
that slab's float32 ball test -- on clouds near the origin, clouds translated by 4096 with rho = 2^-6, |d| from 1e-3 to
1e3, points exactly on the rays, and hair-thin rays forced to the slab cap."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays_oracle as RO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ray_terms") / "libray_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "ray_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _rays(o, d, s_min, s_max):
    o, d = (np.ascontiguousarray(x, f32).reshape(-1, 3) for x in (o, d))
    lo, hi = RO.bounds(len(o), s_min, s_max)
    return o, d, np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def member_pairs(lib, o, d, s_min, s_max, rho, p):
    o, d, lo, hi = _rays(o, d, s_min, s_max)
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    m = len(o)
    us, mem = np.full(m, -1, np.int32), np.full(m, -1, np.int32)
    a, cc = np.zeros(m, f64), np.zeros(m, f64)
    lib.ray_member_batch(_p(o), _p(d), _p(lo), _p(hi), ctypes.c_float(rho), _p(p), ctypes.c_int64(m), _p(us), _p(mem), _p(a),
                         _p(cc))
    return us, mem, a, cc


def _check_pairs(lib, o, d, s_min, s_max, rho, p):
    us, mem, a, cc = member_pairs(lib, o, d, s_min, s_max, rho, p)
    o, d, lo, hi = _rays(o, d, s_min, s_max)
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    want_u = RO.ray_terms(o, d, lo, hi, rho)[4]
    assert np.array_equal(us, want_u.astype(np.int32))
    for f in range(0, len(o), 256):  # the oracle makes all pairs of a block: its diagonal
        e = min(f + 256, len(o))
        m, wa, wcc = RO.members(p[f:e], o[f:e], d[f:e], lo[f:e], hi[f:e], rho)
        k = np.arange(e - f)
        assert np.array_equal(mem[f:e], m[k, k].astype(np.int32))
        assert np.array_equal(a[f:e], wa[k, k], equal_nan=True)
        assert np.array_equal(cc[f:e], wcc[k, k], equal_nan=True)
    return mem


def _near_rays(rng, o, d, rho, s_lo=-0.2, s_hi=1.2):
    """One point near each ray: on it at a random s, pushed sideways by 0 .. 1.5 rho (metric)."""
    o64, d64 = o.astype(f64), d.astype(f64)
    s = rng.uniform(s_lo, s_hi, len(o))
    side = np.cross(d64, rng.normal(size=(len(o), 3)))
    side /= np.maximum(np.linalg.norm(side, axis=1, keepdims=True), 1e-300)
    return (o64 + s[:, None] * d64 + side * (rng.uniform(0.0, 1.5, len(o)) * rho)[:, None]).astype(f32)


def test_member_test_matches_the_oracle_on_random_pairs(host):
    rng = np.random.default_rng(11)
    m = 4000
    o = rng.uniform(-10, 10, (m, 3)).astype(f32)
    d = (rng.normal(size=(m, 3)) * 10.0 ** rng.uniform(-3, 3, (m, 1))).astype(f32)
    rho = 0.25
    p = _near_rays(rng, o, d, rho)
    s_min = rng.uniform(-0.5, 0.3, m).astype(f32)
    s_max = rng.uniform(0.7, 1.5, m).astype(f32)
    mem = _check_pairs(host, o, d, s_min, s_max, rho, p)
    assert 0.2 * m < mem.sum() < 0.8 * m  # both answers are exercised


def test_member_test_on_adversarial_inputs(host):
    nan, inf = np.nan, np.inf
    o = np.zeros((14, 3), f32)
    d = np.tile(np.array([1, 0, 0], f32), (14, 1))
    p = np.tile(np.array([0.5, 0, 0], f32), (14, 1))
    s_min, s_max = np.zeros(14, f32), np.full(14, inf, f32)
    o[0, 1] = nan            # NaN origin
    o[1, 0] = inf            # infinite origin
    d[2] = 0                 # dd == 0
    d[3] = [0, -0.0, 0]      # ... with a negative zero
    d[4, 2] = nan
    d[5, 0] = -inf
    s_min[6] = nan
    s_max[7] = nan
    s_min[8], s_max[8] = 2, 1  # s_min > s_max
    p[9, 1] = nan            # a NaN point
    p[10, 0] = inf           # an infinite point on the axis
    s_min[11], s_max[11] = -inf, inf
    p[11, 0] = -3
    d[12] = [1e-30, 0, 0]    # a tiny direction: dd = 1e-60 is no underflow in float64
    p[12] = [1e-30, 0, 0]
    s_min[13] = s_max[13] = 0.5  # a range of one point
    mem = _check_pairs(host, o, d, s_min, s_max, 0.25, p)
    assert list(mem) == [0] * 11 + [1, 1, 1]


def test_tube_surface_and_range_ends_are_inclusive(host):
    """Dyadic coordinates: every product is exact.  rho = 0.5: a point at offset exactly 0.5 is a member, the next
    float32 above is not; a point at exactly s_min or s_max is a member, its float32 neighbours outside are not."""
    up, dn = np.nextafter(f32(0.5), f32(1)), np.nextafter(f32(0.5), f32(0))
    d = [2, 0, 0]  # not unit: dd = 4
    rows = [  # (p, s_min, s_max, member)
        ([3, 0.5, 0], 0, 4, 1), ([3, up, 0], 0, 4, 0), ([3, 0, -0.5], 0, 4, 1), ([3, 0, -up], 0, 4, 0),
        ([3, 0.5, 0.5], 0, 4, 0), ([3, dn, 0], 0, 4, 1),
        ([1, 0, 0], 0.5, 4, 1), ([np.nextafter(f32(1), f32(0)), 0, 0], 0.5, 4, 0),
        ([8, 0.25, 0], 0, 4, 1), ([np.nextafter(f32(8), f32(9)), 0.25, 0], 0, 4, 0),
        ([-2, 0, 0.5], -1, 4, 1), ([np.nextafter(f32(-2), f32(-3)), 0, 0.5], -1, 4, 0),
    ]
    p = np.array([r[0] for r in rows], f32)
    o = np.zeros_like(p)
    mem = _check_pairs(host, o, np.tile(np.array(d, f32), (len(p), 1)), np.array([r[1] for r in rows], f32),
                       np.array([r[2] for r in rows], f32), 0.5, p)
    assert list(mem) == [r[3] for r in rows]


def test_comparison_matches_the_oracle(host):
    rng = np.random.default_rng(5)
    m = 2000
    a = rng.integers(-3, 4, m).astype(f64)  # many ties
    b = rng.integers(-3, 4, m).astype(f64)
    i = rng.integers(-1, 6, m).astype(np.int32)
    j = rng.integers(-1, 6, m).astype(np.int32)
    out = np.full(m, -1, np.int32)
    host.ray_beats_batch(_p(a), _p(i), _p(b), _p(j), ctypes.c_int64(m), _p(out))
    want = np.array([RO.beats(a[k], i[k], b[k], j[k]) for k in range(m)], np.int32)
    assert np.array_equal(out, want)
    assert RO.beats(1.0, 2, 1.0, 3) and not RO.beats(1.0, 3, 1.0, 2) and not RO.beats(1.0, 3, 1.0, 3)
    assert RO.beats(5.0, 0, 0.0, -1) and not RO.beats(-5.0, -1, 0.0, 7)


def clip(lib, o, d, s_min, s_max, rho, lo, hi, any_point=True):
    o, d, smin, smax = _rays(o, d, s_min, s_max)
    lo, hi = np.ascontiguousarray(lo, f32), np.ascontiguousarray(hi, f32)
    m = len(o)
    ok, a0, a1 = np.full(m, -1, np.int32), np.full(m, 7.0), np.full(m, 7.0)
    lib.ray_clip_batch(_p(o), _p(d), _p(smin), _p(smax), ctypes.c_float(rho), _p(lo), _p(hi), ctypes.c_int32(any_point),
                       ctypes.c_int64(m), _p(ok), _p(a0), _p(a1))
    return ok, a0, a1


def test_box_clip_matches_the_oracle(host):
    rng = np.random.default_rng(23)
    m = 3000
    o = rng.uniform(-30, 30, (m, 3)).astype(f32)
    d = (rng.normal(size=(m, 3)) * 10.0 ** rng.uniform(-3, 3, (m, 1))).astype(f32)
    d[rng.random((m, 3)) < 0.15] = 0  # axis-parallel rays and dd == 0 among them
    o[::97, 0] = np.nan
    s_min = rng.uniform(-2, 1, m).astype(f32)
    s_max = (s_min + rng.uniform(-0.2, 50, m)).astype(f32)
    s_max[::5] = np.inf
    s_min[::7] = -np.inf
    for lo, hi, rho in (([-10, -5, 0], [10, 5, 3], 0.1), ([4090, 4090, 4090], [4100, 4100, 4100], 2.0 ** -6),
                        ([1, 1, 1], [1, 1, 1], 1e-3)):
        aim = rng.uniform(lo, hi, (m, 3)) - o  # every other ray is aimed at the box
        dk = d.copy()
        dk[::2] = (aim * 10.0 ** rng.uniform(-3, 3, (m, 1))).astype(f32)[::2]
        got = clip(host, o, dk, s_min, s_max, rho, lo, hi)
        want = RO.clip(o, dk, s_min, s_max, rho, lo, hi)
        assert np.array_equal(got[0], want[0].astype(np.int32))
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert got[0].sum() > 0.05 * m and (got[0] == 0).sum() > 0.05 * m  # both answers are exercised
    got = clip(host, o, d, s_min, s_max, 0.1, [0, 0, 0], [0, 0, 0], any_point=False)
    assert not got[0].any()


def cover(lib, o, d, s_min, s_max, rho, lo, hi, target, p):
    o, d, smin, smax = _rays(o, d, s_min, s_max)
    lo, hi, p = np.ascontiguousarray(lo, f32), np.ascontiguousarray(hi, f32), np.ascontiguousarray(p, f32).reshape(-1, 3)
    slabs, out = np.zeros(len(o), np.int32), np.zeros(5, np.int64)
    lib.ray_cover_check(_p(o), _p(d), _p(smin), _p(smax), ctypes.c_float(rho), _p(lo), _p(hi), ctypes.c_float(target), _p(p),
                        ctypes.c_int64(len(p)), ctypes.c_int64(len(o)), _p(slabs), _p(out))
    return slabs, dict(zip(("members", "outside_clip", "not_one_owner", "ball_missed", "bad_borders"), map(int, out)))


def _cover_scene(rng, m, per_ray, shift, extent, rho, dscale):
    """m rays through a cloud in shift + [0, extent]^3: random points, points near the rays, and points exactly on the
    rays (computed in float64, rounded to float32) at many s."""
    o = (shift + rng.uniform(-0.5 * extent, 1.5 * extent, (m, 3))).astype(f32)
    e = (shift + rng.uniform(0, extent, (m, 3))).astype(f32)
    d = ((e - o).astype(f64) * 10.0 ** rng.uniform(-dscale, dscale, (m, 1))).astype(f32)
    near = [_near_rays(rng, o, d, rho, 0.0, 2.0 * (np.linalg.norm((e - o).astype(f64), axis=1) /
                                                  np.maximum(np.linalg.norm(d.astype(f64), axis=1), 1e-300)).max())
            for _ in range(per_ray)]
    s = rng.uniform(0, 1, (per_ray, m, 1)) * (np.linalg.norm((e - o).astype(f64), axis=1) /
                                              np.linalg.norm(d.astype(f64), axis=1))[None, :, None] * 1.5
    on = (o.astype(f64)[None] + s * d.astype(f64)[None]).astype(f32).reshape(-1, 3)
    p = np.concatenate(near + [on, (shift + rng.uniform(0, extent, (2000, 3))).astype(f32)])
    p = p[((p >= shift) & (p <= shift + extent)).all(1)]  # the box is the cloud's own
    return o, d, p


@pytest.mark.parametrize("shift,extent,rho,dscale", [(0.0, 10.0, 0.05, 0.0), (0.0, 10.0, 0.05, 3.0),
                                                     (4096.0, 8.0, 2.0 ** -6, 0.0), (4096.0, 8.0, 2.0 ** -6, 3.0),
                                                     (-100000.0, 50.0, 0.01, 1.0), (0.0, 1e-3, 1e-6, 3.0)])
def test_cover_reports_every_member_exactly_once(host, shift, extent, rho, dscale):
    rng = np.random.default_rng(int(abs(shift)) + int(1000 * dscale) + 1)
    o, d, p = _cover_scene(rng, 300, 20, shift, extent, rho, dscale)
    lo, hi = p.min(0), p.max(0)
    for target in (2 * rho, 7.3 * rho):  # a walk's slab length, and a grid cell's
        for s_min, s_max in ((None, None), (-0.25, 0.75)):
            slabs, out = cover(host, o, d, s_min, s_max, rho, lo, hi, target, p)
            assert out["members"] > 1000, out
            assert out["outside_clip"] == 0 and out["not_one_owner"] == 0 and out["ball_missed"] == 0, out
            assert out["bad_borders"] == 0 and slabs.max() > 1


def test_cover_at_the_slab_cap(host):
    """Hair-thin rays (rho = 1e-4) across a cloud 100 units long: 2 rho slabs would be 500 000, the cap lengthens them."""
    cap = ctypes.c_int32()
    host.ray_constants(ctypes.byref(cap))
    assert cap.value == 4096
    rng = np.random.default_rng(3)
    m, rho = 40, 1e-4
    o = np.concatenate([rng.uniform(-1, 0, (m, 1)), rng.uniform(0, 1, (m, 2))], axis=1).astype(f32)
    e = np.concatenate([rng.uniform(100, 101, (m, 1)), rng.uniform(0, 1, (m, 2))], axis=1).astype(f32)
    d = e - o
    s = np.linspace(0.01, 0.99, 3000)[None, :, None]
    on = (o.astype(f64)[:, None] + s * d.astype(f64)[:, None]).astype(f32).reshape(-1, 3)
    p = np.concatenate([on, np.array([[0, 0, 0], [100, 1, 1]], f32)])
    slabs, out = cover(host, o, d, None, None, rho, p.min(0), p.max(0), 2 * rho, p)
    assert (slabs == cap.value).all()
    assert out["members"] > 10000, out  # (float32 rounding puts some of the points outside the hair)
    assert out["outside_clip"] == 0 and out["not_one_owner"] == 0 and out["ball_missed"] == 0 and out["bad_borders"] == 0
