"""csrc/keypoint_terms.h compiled for the host with g++ -ffp-contract=off (tests/cpp/keypoint_terms_host.cpp over the
shim tests/cpp/host_shim): the saliency decision and the "j beats i" predicate the kernels compile give the NumPy
oracle's bits (tests/keypoints_oracle.py) on a table with NaN, +-0, +-inf, equal scores in both id orders and products on
either side of a float32 rounding step, and on random values."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoints_oracle as KO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("keypoint_terms") / "libkeypoint_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "keypoint_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def saliency(lib, eig, g21, g32):
    eig = np.ascontiguousarray(eig, f32).reshape(-1, 3)
    out = np.full(len(eig), -1.0, f32)
    lib.keypoint_saliency_batch(_p(eig), ctypes.c_int64(len(eig)), ctypes.c_float(g21), ctypes.c_float(g32), _p(out))
    return out


def beats(lib, sj, j, si, i):
    sj, si = np.ascontiguousarray(sj, f32), np.ascontiguousarray(si, f32)
    j, i = np.ascontiguousarray(j, np.int64), np.ascontiguousarray(i, np.int64)
    out = np.full(len(sj), -1, np.int32)
    lib.keypoint_beats_batch(_p(sj), _p(j), _p(si), _p(i), ctypes.c_int64(len(sj)), _p(out))
    return out


SPECIAL = np.array([np.nan, -np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.1754944e-38, 0.5, 1.0, np.nextafter(f32(1), f32(2)),
                    3.0, 3.4028235e38, np.inf], f32)


def test_beats_and_candidate_table(host):
    sj, si = (np.array(x, f32) for x in zip(*itertools.product(SPECIAL, SPECIAL)))
    for j, i in ((3, 7), (7, 3), (5, 5), (0, 2 ** 31 - 1), (2 ** 31 - 1, 0)):  # equal scores with both id orders
        jj, ii = np.full(len(sj), j, np.int64), np.full(len(sj), i, np.int64)
        got = beats(host, sj, jj, si, ii)
        assert np.array_equal(got, KO.beats(sj, jj, si, ii).astype(np.int32)), (j, i)
    # by hand: a tie goes to the smaller id, -0 == +0, NaN beats nobody and is beaten by nobody, j == i beats nobody
    assert beats(host, [1, 1, 1, 0.0, np.nan, 1, np.inf, np.inf, 2], [3, 7, 5, 1, 0, 0, 1, 2, 9],
                 [1, 1, 1, -0.0, 1, np.nan, np.inf, np.inf, 1], [7, 3, 5, 2, 1, 1, 2, 1, 0]).tolist() == \
        [1, 0, 0, 1, 0, 0, 1, 0, 1]
    cand = np.full(len(SPECIAL), -1, np.int32)
    host.keypoint_candidate_batch(_p(SPECIAL), ctypes.c_int64(len(SPECIAL)), _p(cand))
    assert np.array_equal(cand, KO.candidate(SPECIAL).astype(np.int32))
    assert cand.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1]


def test_saliency_table(host):
    vals = np.concatenate([SPECIAL, f32([0.1, 0.25, 0.4875, 0.975, 2.0])])
    eig = np.array(list(itertools.product(vals, vals, vals)), f32)
    for g21, g32 in ((0.975, 0.975), (0.5, 0.5), (1.0, 3.0), (1e-30, 1e30)):
        got = saliency(host, eig, g21, g32)
        assert np.array_equal(got.view(np.uint32), KO.saliency(eig, g21, g32).view(np.uint32)), (g21, g32)


def test_saliency_on_either_side_of_a_rounding_step(host):
    """l1 one ulp below, at and one ulp above the float32 product gamma_21 * l2 (and l0 against gamma_32 * l1), for
    products that are not exact in float32: the product is rounded once, then compared strictly"""
    rng = np.random.default_rng(17)
    g = f32(0.975)
    l2 = rng.uniform(0.5, 4.0, 20_000).astype(f32)
    t21 = g * l2
    assert np.any(t21.astype(np.float64) != np.float64(g) * l2.astype(np.float64))
    rows = []
    for l1 in (np.nextafter(t21, f32(0)), t21, np.nextafter(t21, f32(9))):
        t32 = g * l1
        for l0 in (np.nextafter(t32, f32(0)), t32, np.nextafter(t32, f32(9))):
            rows.append(np.stack([l0, l1, l2], axis=1))
    eig = np.concatenate(rows).astype(f32)
    got = saliency(host, eig, g, g)
    want = KO.saliency(eig, g, g)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    n = len(l2)
    assert np.array_equal(got[:n], eig[:n, 0]) and not got[n:].any()  # only (below, below) is salient


def test_random_values(host):
    rng = np.random.default_rng(23)
    eig = np.sort((rng.standard_normal((100_000, 3)) * np.exp(rng.uniform(-20, 20, (100_000, 1)))).astype(f32) ** 2, axis=1)
    assert np.array_equal(saliency(host, eig, 0.975, 0.975).view(np.uint32), KO.saliency(eig, 0.975, 0.975).view(np.uint32))
    s = rng.integers(0, 5, (2, 100_000)).astype(f32)
    ids = rng.integers(0, 50, (2, 100_000))
    assert np.array_equal(beats(host, s[0], ids[0], s[1], ids[1]), KO.beats(s[0], ids[0], s[1], ids[1]).astype(np.int32))
