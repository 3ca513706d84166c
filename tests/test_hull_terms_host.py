"""csrc/hull_terms.h compiled for the host (tests/cpp/hull_terms_host.cpp over the shim tests/cpp/host_shim), once with
g++ -ffp-contract=off and once with contraction on: the exact orientation test against the integer oracle
(tests/hull_oracle.py) on the near-collinear family, on denormals, at the top of the float32 range and under every
permutation of its arguments; which branch answered; the place key's order -- and the measurement of the area and
rectangle errors of the host-compiled finish over the device test's scenes against the contract's derived bounds."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_oracle as HO  # noqa: E402
import hull_scenes as HS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
U53 = 2.0 ** -53

# The contract's bounds (include/pcgx.h, "group footprints"), in units of 2^-53 D^2: the area within 2 h, the
# rectangle's area within 32 of the exact minimum.  Largest figures of the host build over the scenes of
# tests/hull_scenes.py, as test_finish_on_the_scenes measures them (it prints them): area 1.04 (0.104 of its
# bound), rectangle 2.08 (of 32).  The device compiles the same header with contraction off.
AREA_BOUND = lambda h, D: 2 * h * U53 * D * D  # noqa: E731
RECT_BOUND = lambda D: 32 * U53 * D * D  # noqa: E731


@pytest.fixture(scope="module", params=["off", "fast"])
def host(request, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hull_terms_" + request.param) / "libhull_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-variable",
                           "-shared", "-fPIC", "-ffp-contract=" + request.param,
                           "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "hull_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def orient(lib, a, b, c):
    a, b, c = (np.ascontiguousarray(v, f32).reshape(-1, 2) for v in (a, b, c))
    sign, exact, only = (np.zeros(len(a), np.int32) for _ in range(3))
    lib.hull_orient_batch(_p(a), _p(b), _p(c), ctypes.c_int64(len(a)), _p(sign), _p(exact), _p(only))
    return sign, exact, only


def exact_signs(a, b, c):
    A, B, C = (np.asarray(v, f32).reshape(-1, 2) for v in (a, b, c))
    return np.array([HO.orient(HO.integers(p), HO.integers(q), HO.integers(r)) for p, q, r in zip(A, B, C)], np.int32)


def family(k):
    i, j = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    a = np.stack([f32(0.5) + (i.ravel() * 2.0 ** -24).astype(f32), f32(0.5) + (j.ravel() * 2.0 ** -24).astype(f32)], axis=1)
    b = np.full((1024, 2), 12 * 2.0 ** k, f32)
    c = np.full((1024, 2), 24 * 2.0 ** k, f32)
    return a.astype(f32), b, c, i.ravel() == j.ravel()


def plain_f64_signs(a, b, c):
    a, b, c = (v.astype(np.float64) for v in (a, b, c))
    d = (a[:, 0] - c[:, 0]) * (b[:, 1] - c[:, 1]) - (a[:, 1] - c[:, 1]) * (b[:, 0] - c[:, 0])
    return np.sign(d).astype(np.int32)


@pytest.mark.parametrize("k,uncertain,wrong", [(0, 32, 0), (24, 278, 16), (26, 884, 152), (30, 1024, 992), (40, None, None)])
def test_orient_on_the_near_collinear_family(host, k, uncertain, wrong):
    a, b, c, diag = family(k)
    want = exact_signs(a, b, c)
    sign, exact, only = orient(host, a, b, c)
    assert np.array_equal(sign, want) and np.array_equal(only, want)
    assert np.array_equal(want == 0, diag)  # a on the diagonal exactly when i = j
    print("k = %d: %d of 1024 left to the exact branch, plain float64 wrong on %d" % (k, exact.sum(), (plain_f64_signs(a, b, c) != want).sum()))
    if uncertain is not None:
        assert exact.sum() == uncertain and (plain_f64_signs(a, b, c) != want).sum() == wrong
    if k == 0:
        assert np.array_equal(exact == 1, diag)  # the filter gives up only on the exact zeros
    if k == 26:
        assert exact.sum() >= 1


def test_orient_on_denormals_the_top_of_the_range_and_permutations(host):
    rng = np.random.default_rng(5)
    tiny = (rng.integers(-3, 4, (300, 6)) * 2.0 ** -149).astype(f32)  # denormals, many collinear triples among them
    huge = (rng.choice([-1.0, 1.0], (300, 6)) * rng.choice([3e38, 2.9999e38, 1.5e38, 1e38], (300, 6))).astype(f32)
    mixed = np.where(rng.random((300, 6)) < 0.5, tiny, huge).astype(f32)
    line = np.stack([rng.integers(-5, 6, 300) * v for v in (3e37, 1e37, 3e37, 1e37, 3e37, 1e37)], axis=1).astype(f32)
    for name, T in (("denormals", tiny), ("huge", huge), ("mixed", mixed), ("a coarse lattice", line)):
        pts = T.reshape(-1, 3, 2)
        base = exact_signs(pts[:, 0], pts[:, 1], pts[:, 2])
        assert (base == 0).any() or name in ("huge", "mixed"), name
        for perm in itertools.permutations(range(3)):
            parity = 1 if perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)) else -1
            sign, exact, only = orient(host, pts[:, perm[0]], pts[:, perm[1]], pts[:, perm[2]])
            assert np.array_equal(sign, parity * base) and np.array_equal(only, parity * base), (name, perm)


def test_place_keys_order_places_as_less_than_does(host):
    v = f32([-np.inf, -3.4028235e38, -1.0, -1.1754944e-38, -1e-45, -0.0, 0.0, 1e-45, 1.1754944e-38, 1.0, 3.4028235e38, np.inf])
    xy = np.array([(x, y) for x in v for y in v], f32)
    key, back = np.zeros(len(xy), np.uint64), np.zeros((len(xy), 2), f32)
    host.hull_keys(_p(xy), ctypes.c_int64(len(xy)), _p(key), _p(back))
    assert np.array_equal(back, xy)  # (== : a zero decodes as +0)
    assert not np.signbit(back[xy == 0]).any()
    key = [int(k) for k in key]
    assert max(key) < 2 ** 64 - 1  # all ones stays free for a slot that is out
    for (ax, ay), ka in zip(xy, key):
        for (bx, by), kb in zip(xy, key):
            less = ax < bx or (ax == bx and ay < by)
            assert (ka < kb) == less and (ka == kb) == (ax == bx and ay == by)
    a, b = xy[:-1].copy(), xy[1:].copy()
    same = np.zeros(len(a), np.int32)
    host.hull_same_place_batch(_p(a), _p(b), ctypes.c_int64(len(a)), _p(same))
    assert np.array_equal(same == 1, (a == b).all(axis=1)) and same.sum() > 0  # (-0, y) and (+0, y) among them


def finish(lib, v):
    v = np.ascontiguousarray(v, f32).reshape(-1, 2)
    area, rect = np.zeros(1), np.zeros(6)
    lib.hull_finish_host(_p(v), ctypes.c_int64(len(v)), _p(area), _p(rect))
    return area[0], rect


def test_finish_known_answers(host):
    a, r = finish(host, [[0, 0], [4, 0], [4, 3], [0, 3]])
    assert a == 12.0 and r.tolist() == [2.0, 1.5, 1.0, 0.0, 2.0, 1.5]  # a tie of all four edges: the first one
    a, r = finish(host, [[1, 1], [4, 5]])
    assert a == 0 and r.tolist() == [2.5, 3.0, 0.6, 0.8, 2.5, 0.0]
    a, r = finish(host, [[7, -2]])
    assert a == 0 and r.tolist() == [7.0, -2.0, 1.0, 0.0, 0.0, 0.0]
    a, r = finish(host, np.zeros((0, 2)))
    assert a == 0 and not r.any()
    a, r = finish(host, [[-8, 19], [10, -5], [58, 31]])  # tests/test_hull_oracle.py's L: the rectangle lies along the arms
    assert a == 900.0 and abs(r[4] * r[5] * 4 - 1800.0) < 1e-9 and sorted(np.abs(r[2:4]).round(12).tolist()) == [0.6, 0.8]


def test_finish_on_the_scenes(host):
    """the host-compiled finish over the oracle's hulls of the device test's scenes: area and rectangle within the
    contract's derived bounds; prints the largest errors in units of 2^-53 D^2"""
    worst_a = worst_share = worst_r = 0.0
    for name, (pts, ids, sizes) in HS.scenes():
        F, info = HO.group_hulls(pts, ids, sizes)
        for g, v in enumerate(info["hulls"]):
            D, h = info["D"][g], len(v)
            a, r = finish(host, v)
            if h < 3:
                assert a == 0 and r[5] == 0
                continue
            ea, er = abs(a - F.area[g]), 4 * r[4] * r[5] - F.rect_area[g]
            assert ea <= AREA_BOUND(h, D) and er <= RECT_BOUND(D), (name, g, ea, er)
            assert er >= -RECT_BOUND(D)  # (no rectangle along an edge is smaller than the smallest)
            worst_a, worst_share = max(worst_a, ea / (U53 * D * D)), max(worst_share, ea / AREA_BOUND(h, D))
            worst_r = max(worst_r, abs(er) / (U53 * D * D))
    print("area: largest error %.3g x 2^-53 D^2, %.3g of its bound; rectangle: %.3g x 2^-53 D^2" % (worst_a, worst_share, worst_r))
