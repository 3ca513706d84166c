"""csrc/dbscan_terms.h compiled for the host with g++ -ffp-contract=off (tests/cpp/dbscan_terms_host.cpp over the shim
tests/cpp/host_shim): the nearest-core comparison and the core test the kernels compile give the NumPy oracle's answers
(tests/dbscan_oracle.py) over equal distances, equal ids, +-0, denormals and NaN distances, and at min_pts - 1, min_pts
and min_pts + 1."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dbscan_oracle as DO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dbscan_terms") / "libdbscan_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "dbscan_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def beats(lib, d, i, bd, bi):
    d, bd = np.ascontiguousarray(d, f32), np.ascontiguousarray(bd, f32)
    i, bi = np.ascontiguousarray(i, np.uint32), np.ascontiguousarray(bi, np.uint32)
    out = np.full(len(d), -1, np.int32)
    lib.dbscan_beats_batch(_p(d), _p(i), _p(bd), _p(bi), ctypes.c_int64(len(d)), _p(out))
    return out


DIST = np.array([np.nan, -0.0, 0.0, 1e-45, 3e-45, 1.1754942e-38, 1.1754944e-38, 0.25, np.nextafter(f32(0.25), f32(1)), 1.0,
                 3.4028235e38, np.inf], f32)
IDS = np.array([0, 1, 2, 7, 0x7ffffffe, 0x7fffffff, 0xffffffff], np.uint32)


def test_beats_table(host):
    rows = np.array(list(itertools.product(range(len(DIST)), range(len(IDS)), range(len(DIST)), range(len(IDS)))))
    d, i, bd, bi = DIST[rows[:, 0]], IDS[rows[:, 1]], DIST[rows[:, 2]], IDS[rows[:, 3]]
    got = beats(host, d, i, bd, bi)
    want = np.array([DO.beats(*r) for r in zip(d, i, bd, bi)], np.int32)
    assert np.array_equal(got, want)
    assert 0 < got.sum() < len(got)
    with np.errstate(invalid="ignore"):
        nan_side = np.isnan(d) | np.isnan(bd)
    assert not got[nan_side].any()                         # a NaN beats nobody, and nobody beats a NaN
    assert not got[(rows[:, 0] == rows[:, 2]) & (rows[:, 1] == rows[:, 3])].any()  # nobody beats itself
    # a strict order on the candidates without a NaN: exactly one of two different ones beats the other
    back = beats(host, bd, bi, d, i)
    diff = ~nan_side & ~((d == bd) & (i == bi))
    assert np.all(got[diff] + back[diff] == 1)


def test_beats_by_hand(host):
    def one(d, i, bd, bi):
        return beats(host, [d], [i], [bd], [bi]).tolist()[0]
    assert one(0.5, 9, 0.75, 1) == 1 and one(0.75, 1, 0.5, 9) == 0       # the distance first
    assert one(0.5, 1, 0.5, 2) == 1 and one(0.5, 2, 0.5, 1) == 0          # equal distances: the smaller id
    assert one(0.5, 2, 0.5, 2) == 0
    assert one(-0.0, 1, 0.0, 2) == 1 and one(0.0, 2, -0.0, 1) == 0        # -0 == +0: the id decides
    assert one(0.0, 1, -0.0, 2) == 1
    assert one(1e-45, 5, 3e-45, 0) == 1 and one(3e-45, 0, 1e-45, 5) == 0  # denormals are not flushed
    assert one(0.0, 5, 1e-45, 0) == 1
    assert one(np.nan, 0, np.inf, 0xffffffff) == 0 and one(1.0, 0, np.nan, 9) == 0
    assert one(3.4028235e38, 0x7fffffff, np.inf, 0xffffffff) == 1         # any candidate beats the initial best


@pytest.mark.parametrize("min_pts", [1, 2, 4, 64, 0x7fffffff])
def test_core_round_min_pts(host, min_pts):
    count = np.array(sorted({0, 1, max(min_pts - 1, 0), min_pts, min(min_pts + 1, 0xffffffff), 0xffffffff}), np.uint32)
    for own in (0, 1):
        o = np.full(len(count), own, np.int32)
        out = np.full(len(count), -1, np.int32)
        host.dbscan_core_batch(_p(o), _p(count), ctypes.c_int32(min_pts), ctypes.c_int64(len(count)), _p(out))
        want = np.array([DO.is_core(own, c, min_pts) for c in count], np.int32)
        assert np.array_equal(out, want), (min_pts, own)
        assert np.array_equal(out, ((count.astype(np.int64) >= min_pts) & (own == 1)).astype(np.int32))
    kinds = (ctypes.c_int32 * 3)()
    host.dbscan_kinds(kinds)
    assert list(kinds) == [DO.NOISE, DO.BORDER, DO.CORE] == [0, 1, 2]
