"""csrc/ground_terms.h compiled for the host with g++ -ffp-contract=off (tests/cpp/ground_terms_host.cpp over the shim
tests/cpp/host_shim): the cell of a point, the live test, the key round trip, the empty encodings of the two halves of an
opening and the ground test that the kernels of ground.hip compile give the NumPy oracle's answers (tests/ground_oracle.py)
on random points, points on cell borders, the far edge where fx == nx, +-0, denormals, NaN and infinities."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_oracle as GO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ground_terms") / "libground_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "ground_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def cells(lib, pts, origin, dims, cell):
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    o, d = np.ascontiguousarray(origin, f32), np.ascontiguousarray(dims, np.int32)
    out = np.full(len(pts), -7, np.int32)
    lib.ground_cell_batch(_p(pts), ctypes.c_int64(len(pts)), _p(o), _p(d), ctypes.c_float(cell), _p(out))
    return out


def test_constants(host):
    out = (ctypes.c_uint32 * 2)()
    host.ground_constants(out)
    assert list(out) == [int(GO.EMPTY), 0x7FC00000]


def test_cells_of_random_points(host):
    rng = np.random.default_rng(2)
    for origin, dims, cell in (((0, 0), (10, 7), 1.0), ((-3.25, 11.5), (33, 129), 0.3), ((1e4, -1e4), (8192, 8192), 0.01),
                               ((0.1, 0.2), (1, 1), 5.0)):
        ext = np.array([dims[0] * cell, dims[1] * cell, 10.0])
        pts = (rng.random((4000, 3)) * ext * 1.2 - ext * 0.1 + [origin[0], origin[1], 0]).astype(f32)
        got = cells(host, pts, origin, dims, cell)
        assert np.array_equal(got, GO.cells(pts, origin, dims, cell))
        assert (got >= 0).sum() > 1000 and (got < 0).sum() > 100 and got.max() < dims[0] * dims[1]


def test_cell_borders_and_the_far_edge(host):
    # unit cells from 0: a point ON a border belongs to the cell that begins there; x == nx * cell is outside (fx == nx)
    pts = np.array([[0, 0, 0], [1, 0, 0], [0.99999994, 0, 0], [3, 0, 0], [2.9999998, 0, 0], [0, 2, 0], [0, 1.9999999, 0],
                    [-0.0, -0.0, 0], [-1e-45, 0, 0], [2, 1, 0]], f32)
    got = cells(host, pts, (0, 0), (3, 2), 1.0)
    assert list(got) == [0, 1, 0, -1, 2, -1, 3, 0, -1, 5]
    # a cell size that does not divide evenly: the quotient's rounding decides, in float32, as the oracle's does
    x = (np.arange(0, 400) * 0.1 + 0.05).astype(f32)  # the borders of the cells of a grid from 0.05
    pts = np.stack([x, x[::-1], np.zeros_like(x)], axis=1)
    got = cells(host, pts, (0.05, 0.05), (400, 400), 0.1)
    assert np.array_equal(got, GO.cells(pts, (0.05, 0.05), (400, 400), 0.1))
    assert (got >= 0).all()


def test_not_live(host):
    bad = [np.nan, np.inf, -np.inf]
    pts = np.array([[b if k == j else 0.5 for k in range(3)] for b in bad for j in range(3)] +
                   [[3e38, 0.5, 0], [-3e38, 0.5, 0], [0.5, 0.5, 3e38], [0.5, 0.5, -1e-42]], f32)
    got = cells(host, pts, (-3e38, 0), (5, 5), 1.0)  # x - ox overflows for the first of the finite ones
    want = GO.cells(pts, (-3e38, 0), (5, 5), 1.0)
    assert np.array_equal(got, want) and np.all(got[:10] == -1) and got[10] == 0
    got = cells(host, pts, (0, 0), (5, 5), 1.0)
    assert list(got[9:]) == [-1, -1, 0, 0] and np.all(got[:9] == -1)


def test_key_round_trip(host):
    rng = np.random.default_rng(4)
    z = np.concatenate([rng.standard_normal(2000) * 100, [0.0, -0.0, 1e-45, -1e-45, 3.4e38, -3.4e38, 1e-38, -1e-38]]).astype(f32)
    key, back, surf = np.zeros(len(z), np.uint32), np.zeros(len(z), f32), np.zeros(len(z), f32)
    host.ground_key_batch(_p(z), ctypes.c_int64(len(z)), _p(key), _p(back), _p(surf))
    assert np.array_equal(key, GO.key(z))
    assert np.array_equal(back.view(np.uint32), z.view(np.uint32)) and np.array_equal(surf.view(np.uint32), z.view(np.uint32))
    assert len(np.unique(key)) == len(np.unique(z.view(np.uint32)))
    assert np.all(np.diff(z[np.argsort(key)]) >= 0)  # the keys' order is the floats'
    assert key[2000] > key[2001]  # +0.0 above -0.0
    assert not np.any(key == GO.EMPTY) and not np.any(key == 0)


def test_empty_encodings(host):
    words = np.array([0xFFFFFFFF, GO.key(f32(1.5))[0], 0xFFFFFFFF, 0xFFFFFFFF, GO.key(f32(-2.0))[0], GO.key(f32(-0.0))[0]],
                     np.uint32)
    m = len(words)
    for is_max in (0, 1):
        i, o, op = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        host.ground_morph_batch(_p(words), ctypes.c_int64(m), ctypes.c_int32(is_max), _p(i), _p(o), _p(op))
        assert np.array_equal(o, words)  # through a pass and back: the word in memory
        nxt = np.roll(words, -1)
        if is_max:
            a, b = np.where(words == GO.EMPTY, 0, words), np.where(nxt == GO.EMPTY, 0, nxt)
            assert np.array_equal(i, a) and np.array_equal(op, np.maximum(a, b))
        else:
            assert np.array_equal(i, words) and np.array_equal(op, np.minimum(words, nxt))
    surf = np.zeros(1, f32)
    key, back = np.zeros(1, np.uint32), np.zeros(1, f32)
    host.ground_key_batch(_p(np.array([np.inf], f32)), ctypes.c_int64(1), _p(key), _p(back), _p(surf))
    assert key[0] != GO.EMPTY  # (+inf is no live point's z, and still not the empty word)


def test_ground_test(host):
    rng = np.random.default_rng(6)
    s = (rng.standard_normal(3000) * 5).astype(f32)
    ht = (rng.random(3000) * 2 + 0.01).astype(f32)
    z = (s + rng.random(3000).astype(f32) * 3).astype(f32)
    z[:500] = (s[:500] + ht[:500]).astype(f32)  # at the bound, give or take the rounding of the sum
    z[500:520] = s[500:520]
    s[520:524], z[520:524], ht[520:524] = [-3e38, 0.0, -0.0, 1.0], [3e38, -0.0, 0.0, 1.25], [1.0, 1e-45, 1e-45, 0.25]
    surv, hag = np.zeros(3000, np.int32), np.zeros(3000, f32)
    host.ground_test_batch(_p(z), _p(s), _p(ht), ctypes.c_int64(3000), _p(surv), _p(hag))
    with np.errstate(all="ignore"):
        want = z - s
    assert np.array_equal(hag.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(surv, (want < ht).astype(np.int32))
    assert 50 < surv[:500].sum() < 450  # both sides of the strict comparison
    assert list(surv[520:524]) == [0, 1, 1, 0]  # an overflow fails; zeros of either sign are 0 apart; equality fails
