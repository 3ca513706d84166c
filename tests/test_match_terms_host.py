"""csrc/fpfh_match_terms.h compiled for the host with g++ -ffp-contract=off (tests/cpp/match_terms_host.cpp over the
shim tests/cpp/host_shim): the row distance and the usable test the kernels compile give the NumPy oracle's bits
(tests/match_oracle.py) on 1e5 random row pairs and on the rows worked by hand (tests/test_match_oracle.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_oracle as MO  # noqa: E402
from test_match_oracle import A_HAND, B_HAND, hand_pairs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("match_terms") / "libmatch_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "match_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def dist(lib, a, b):
    a, b = (np.ascontiguousarray(x, f32).reshape(-1, MO.LEN) for x in (a, b))
    D = np.full(len(a), -1.0, f32)
    lib.match_dist_batch(_p(a), _p(b), ctypes.c_int64(len(a)), _p(D))
    return D


def usable(lib, a):
    a = np.ascontiguousarray(a, f32).reshape(-1, MO.LEN)
    u = np.full(len(a), -1, np.int32)
    lib.match_usable_batch(_p(a), ctypes.c_int64(len(a)), _p(u))
    return u


def _oracle_pairs(a, b):
    """the oracle's loop, pair by pair instead of all against all"""
    acc = np.zeros(len(a), f32)
    with np.errstate(over="ignore"):
        for k in range(MO.LEN):
            d = a[:, k] - b[:, k]
            acc = acc + d * d
    return acc


def test_constants_are_the_headers(host):
    assert host.match_len() == MO.LEN == 33


def test_random_pairs(host):
    A, B = MO.scene_r(50_000, 50_000, seed=11)
    rng = np.random.default_rng(3)
    a = np.concatenate([A, (rng.standard_normal((50_000, 33)) * np.exp(rng.uniform(-20, 20, (50_000, 1)))).astype(f32)])
    b = np.concatenate([B, (rng.standard_normal((50_000, 33)) * np.exp(rng.uniform(-20, 20, (50_000, 1)))).astype(f32)])
    want = _oracle_pairs(a, b)
    assert np.array_equal(want[:64], np.diag(MO.dist_matrix(a[:64], b[:64])))  # (the pairwise form is the matrix's)
    got = dist(host, a, b)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dist(host, b, a).view(np.uint32), want.view(np.uint32))  # D(a, b) == D(b, a), bit for bit
    assert np.array_equal(usable(host, a), MO.usable(a).astype(np.int32)) and usable(host, a).all()


def test_hand_rows(host):
    a, b, D = hand_pairs()
    assert np.array_equal(dist(host, a, b).view(np.uint32), D.view(np.uint32))
    assert np.array_equal(dist(host, b, a).view(np.uint32), D.view(np.uint32))
    for rows in (A_HAND, B_HAND):
        assert np.array_equal(usable(host, rows), MO.usable(rows).astype(np.int32))
    assert usable(host, B_HAND).tolist() == [1, 1, 1, 0, 0, 0, 0]
    # every position decides: one non-zero value makes a row usable, one NaN or inf unusable, wherever it stands
    for k in range(MO.LEN):
        r = np.zeros((3, MO.LEN), f32)
        r[0, k] = -1e-40  # a denormal is not zero
        r[1] = 1.0
        r[1, k] = np.nan
        r[2] = 1.0
        r[2, k] = -np.inf
        assert usable(host, r).tolist() == [1, 0, 0] == MO.usable(r).astype(int).tolist(), k
