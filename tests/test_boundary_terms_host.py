"""csrc/boundary_terms.h compiled for the host with g++ -ffp-contract=off (tests/cpp/boundary_terms_host.cpp over the
shim tests/cpp/host_shim): the frame of a normal, the evaluated test, a and b of a neighbour, the sector and the gap of a
mask that the kernel compiles give the NumPy oracle's answers (tests/boundary_oracle.py), by array_equal, on random
inputs, the lattice's border directions, normals with tied smallest components, +-0 components, denormals, NaN and
+-inf, and a == b == 0."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_oracle as BO  # noqa: E402
import boundary_scenes as BS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, u64 = np.float32, np.float64, np.uint64


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("boundary_terms") / "libboundary_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "boundary_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def frames(lib, n):
    n = np.ascontiguousarray(n, f32).reshape(-1, 3)
    ok, fr = np.full(len(n), -1, np.int32), np.zeros((len(n), 6), f64)
    lib.boundary_frame_batch(_p(n), ctypes.c_int64(len(n)), _p(ok), _p(fr))
    return ok, fr


def directions(lib, n, p, q):
    n, p, q = (np.ascontiguousarray(x, f32).reshape(-1, 3) for x in (n, p, q))
    ab, sec = np.zeros((len(n), 2), f64), np.full(len(n), -9, np.int32)
    lib.boundary_direction_batch(_p(n), _p(p), _p(q), ctypes.c_int64(len(n)), _p(ab), _p(sec))
    return ab, sec


def sectors(lib, a, b):
    a, b = np.ascontiguousarray(a, f64), np.ascontiguousarray(b, f64)
    out = np.full(len(a), -9, np.int32)
    lib.boundary_sector_batch(_p(a), _p(b), ctypes.c_int64(len(a)), _p(out))
    return out


def gaps(lib, m):
    m = np.ascontiguousarray(m, u64)
    out = np.full(len(m), -9, np.int32)
    lib.boundary_gap_batch(_p(m), ctypes.c_int64(len(m)), _p(out))
    return out


def _check_frames(lib, n):
    n = np.ascontiguousarray(n, f32).reshape(-1, 3)
    ok, fr = frames(lib, n)
    want = BO.usable(n)
    assert np.array_equal(ok, want.astype(np.int32))
    u, v = BO.frame(n)
    assert np.array_equal(fr[want, :3], u[want]) and np.array_equal(fr[want, 3:], v[want])  # (a frame is used only then)
    return ok, fr


def test_constants(host):
    sec, tans = ctypes.c_int32(), np.zeros(16, f64)
    host.boundary_constants(ctypes.byref(sec), _p(tans))
    assert sec.value == BO.SECTORS == 64
    assert np.array_equal(tans, BO.T)  # the header's 15 hex literals are the oracle's 15 numbers


def test_frames_of_special_normals(host):
    vals = f32([0.0, -0.0, 1e-45, -1e-45, 1.1754944e-38, 0.5, -0.5, 1.0, -1.0, 3.4028235e38, np.nan, np.inf, -np.inf])
    n = np.array(list(itertools.product(vals, vals, vals)), f32)  # every tie of the smallest component among them
    ok, fr = _check_frames(host, n)
    assert 0 < ok.sum() < len(n)
    assert not ok[np.all(n == 0, axis=1)].any() and not ok[~np.isfinite(n).all(axis=1)].any()
    # by hand: a three-way tie and a tie of x and y take the x axis, a tie of y and z the y axis
    _, fr = frames(host, [[1, 1, 1], [0.5, 0.5, 1], [1, 0.5, 0.5], [0, 0, 1], [0, 0, -1]])
    assert fr[:, :3].tolist() == [[0, 1, -1], [0, 1, -0.5], [-0.5, 0, 1], [0, 1, 0], [0, -1, 0]]
    assert fr[3:, 3:].tolist() == [[-1, 0, 0], [-1, 0, 0]]


def test_random_frames_directions_and_sectors(host):
    rng = np.random.default_rng(11)
    m = 200_000
    n = rng.standard_normal((m, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)
    n[: m // 4] *= np.exp(rng.uniform(-40, 40, (m // 4, 1))).astype(f32)  # not of unit length: the same arithmetic
    n = n[BO.usable(n)]
    m = len(n)
    _check_frames(host, n)
    q = (rng.random((m, 3)) * 100 - 50).astype(f32)
    p = (q + rng.standard_normal((m, 3)) * np.exp(rng.uniform(-12, 3, (m, 1)))).astype(f32)
    p[::7] = q[::7]  # the point itself
    ab, sec = directions(host, n, p, q)
    u, v = BO.frame(n)
    a, b = BO.direction(u, v, p, q)
    assert np.array_equal(ab[:, 0], a) and np.array_equal(ab[:, 1], b)
    want = BO.sector(a, b)
    assert np.array_equal(sec, want)
    assert np.all(want[::7] == -1) and len(np.unique(want)) == 65
    # neighbours on the normal's line have no direction (axis-aligned normals: the products are exact)
    ax = np.tile(f32([[0, 0, 1], [0, -1, 0], [2, 0, 0]]), (50, 1))
    qq = (rng.integers(-64, 64, (150, 3)) / 8.0).astype(f32)
    pp = (qq + ax * (rng.integers(1, 9, (150, 1)) / 8.0).astype(f32)).astype(f32)
    assert np.all(directions(host, ax, pp, qq)[1] == -1)


def test_lattice_border_directions(host):
    """the eight neighbours of a lattice point lie exactly on sector borders, under both normals"""
    pts, _ = BS.lattice()
    q = np.tile(pts[24], (8, 1))  # the middle
    nb = pts[[31, 32, 25, 18, 17, 16, 23, 30]]
    for nz in (1.0, -1.0):
        n = np.tile(f32([0, 0, nz]), (8, 1))
        ab, sec = directions(host, n, nb, q)
        u, v = BO.frame(n)
        assert np.array_equal(sec, BO.sector(*BO.direction(u, v, nb, q)))
        assert sorted(sec.tolist()) == [0, 8, 16, 24, 32, 40, 48, 56]


def test_sectors_at_borders_and_zeros(host):
    rng = np.random.default_rng(12)
    # directions on, just below and just above every border x T[k] of every quarter, at many scales
    x = np.exp(rng.uniform(-200, 200, 4000))
    rows = []
    for k in range(0, 16):
        y = x * BO.T[k]
        for yy in (np.nextafter(y, -np.inf), y, np.nextafter(y, np.inf)):
            yy = np.maximum(yy, 0.0)
            rows += [(x, yy), (-yy, x), (-x, -yy), (yy, -x)]
    a = np.concatenate([r[0] for r in rows])
    b = np.concatenate([r[1] for r in rows])
    got = sectors(host, a, b)
    assert np.array_equal(got, BO.sector(a, b)) and len(np.unique(got)) == 64
    z = f64([0.0, -0.0])
    a, b = (np.array(v, f64) for v in zip(*itertools.product(np.concatenate([z, [1.0, -1.0, 5e-324, -5e-324, 1e308, -1e308]]),
                                                             repeat=2)))
    got = sectors(host, a, b)
    assert np.array_equal(got, BO.sector(a, b))
    assert np.array_equal(got == -1, (a == 0) & (b == 0)) and (got == -1).sum() == 4


def test_evaluated(host):
    rows = np.array(list(itertools.product((0, 1), (0, 1), (0, 1, 2, 5, 2 ** 31 - 1), (-2 ** 31, -1, 0, 1, 2, 5, 6, 2 ** 31 - 1))),
                    np.int32)
    met, ok, cnt, mn = (np.ascontiguousarray(rows[:, k]) for k in range(4))
    out = np.full(len(rows), -1, np.int32)
    host.boundary_evaluated_batch(_p(met), _p(ok), _p(cnt), _p(mn), ctypes.c_int64(len(rows)), _p(out))
    want = (met == 1) & (ok == 1) & (cnt.astype(np.int64) >= np.maximum(mn.astype(np.int64), 1))
    assert np.array_equal(out, want.astype(np.int32)) and 0 < want.sum() < len(want)


def test_gaps(host):
    pat = np.arange(1 << 16, dtype=u64)
    rep = pat | (pat << u64(16)) | (pat << u64(32)) | (pat << u64(48))
    assert np.array_equal(gaps(host, rep), BO.gap(rep))
    rng = np.random.default_rng(13)
    rnd = rng.integers(0, 1 << 63, (200_000, 6), dtype=np.uint64) << u64(1) | rng.integers(0, 2, (200_000, 6), dtype=np.uint64)
    k = rng.integers(1, 7, 200_000)
    m = rnd[:, 0].copy()
    for j in range(1, 6):
        m = np.where(k > j, m & rnd[:, j], m)
    got = gaps(host, m)
    assert np.array_equal(got, BO.gap(m)) and len(np.unique(got)) > 30
    edge = np.array([0, 0xFFFFFFFFFFFFFFFF] + [1 << s for s in range(64)] + [0xFFFFFFFFFFFFFFFF ^ (1 << s) for s in range(64)], u64)
    assert gaps(host, edge).tolist() == [64, 0] + [63] * 64 + [1] * 64
    # every cyclic run: `run` zero bits from `at` on, ones elsewhere
    for run in range(1, 64):
        at = np.arange(64, dtype=u64)
        ones = u64((1 << run) - 1)
        hole = (ones << at) | (ones >> (u64(64) - at) % u64(64)) * (at > 0)
        assert np.all(gaps(host, ~hole) == run), run
