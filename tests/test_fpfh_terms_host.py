"""csrc/fpfh_terms.h compiled for the host with g++ (tests/cpp/fpfh_terms_host.cpp over the shim
tests/cpp/host_shim), twice: -ffp-contract=off and -ffp-contract=fast with FMA instructions where the CPU has them.

Per pair against the NumPy oracle (tests/fpfh_oracle.py) on 1e5 random pairs and on the crafted ones
(tests/test_fpfh_oracle.py: worked by hand, the clamps, an edge, a swap tie, invalid pairs): the bins lie in the pair's
admissible set, and the validity flag equals the oracle's wherever the pair is not fragile.  Whether the header is
compiled with or without contraction must not matter: both variants pass the same checks, and on the random pairs --
none of which is fragile -- that makes their bins equal."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_oracle as FO  # noqa: E402
from test_fpfh_oracle import hand_arrays  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def _cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(" fma " in line + " " for line in f if line.startswith("flags"))
    except OSError:
        return False


VARIANTS = {"off": ["-ffp-contract=off"], "fast": ["-ffp-contract=fast"] + (["-mfma"] if _cpu_has_fma() else [])}


@pytest.fixture(scope="module", params=sorted(VARIANTS))
def host(request, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fpfh_" + request.param) / "libfpfh_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC"]
                          + VARIANTS[request.param] +
                          ["-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "fpfh_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run(lib, ps, ns, pt, nt):
    ps, ns, pt, nt = (np.ascontiguousarray(a, f32).reshape(-1, 3) for a in (ps, ns, pt, nt))
    m = len(ps)
    valid = np.full(m, -1, np.int32)
    bins = np.full((m, 3), -7, np.int32)  # (a sentinel: rows of invalid pairs must keep it)
    lib.fpfh_terms_batch(_p(ps), _p(ns), _p(pt), _p(nt), ctypes.c_int64(m), _p(valid), _p(bins))
    return valid, bins


def _check(lib, ps, ns, pt, nt):
    valid, bins = run(lib, ps, ns, pt, nt)
    pb = FO.pair_bins(ps, ns, pt, nt)
    assert np.all((valid == 0) | (valid == 1))
    v = valid == 1
    assert np.all(v[pb["sure"]])
    assert not np.any(v[~(pb["sure"] | pb["maybe"])])
    assert np.all(bins[~v] == -7)
    assert np.all((bins[v] >= 0) & (bins[v] <= 10))
    rows = np.nonzero(v)[0]
    for f in range(3):
        assert np.all(pb["adm"][rows, f, bins[rows, f]]), (f, rows[~pb["adm"][rows, f, bins[rows, f]]][:5])
    return v, bins, pb


def _random_pairs(m=100_000):
    rng = np.random.default_rng(7)
    ps = rng.uniform(-2, 2, (m, 3)).astype(f32)
    off = rng.standard_normal((m, 3))
    off *= (rng.uniform(0.005, 0.2, m) / np.linalg.norm(off, axis=1))[:, None]
    pt = (ps + off).astype(f32)
    n = rng.standard_normal((2, m, 3))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    return ps, n[0].astype(f32), pt, n[1].astype(f32)


def test_constants_are_the_headers(host):
    assert host.fpfh_len() == FO.LEN == 3 * FO.BINS


def test_random_pairs(host):
    pairs = _random_pairs()
    v, bins, pb = _check(host, *pairs)
    assert v.all() and pb["sure"].all()
    print("fragile pairs among %d random ones: %d" % (len(v), int(pb["fragile"].sum())))
    assert pb["fragile"].sum() <= 2  # (1e5 pairs x 33 edges x 2e-9 wide: 0.007 expected)
    plain = ~pb["fragile"]
    assert np.array_equal(bins[plain], pb["bins"][plain])
    for f in range(3):  # the pairs reach every bin of every feature
        assert len(np.unique(bins[:, f])) == 11


def test_crafted_pairs(host):
    ps, ns, pt, nt = hand_arrays()
    v, bins, pb = _check(host, ps, ns, pt, nt)
    assert np.array_equal(v, pb["sure"]) and np.array_equal(bins[v], pb["bins"][v])
    assert v.tolist() == [True] * 4 + [False] * 4
    # an edge that is a swap tie too (|d| = 11, a1 = a2 = 7 / 11: bin 8 or 9), normals of unequal length, f3 = +-1 a
    # rounding off
    z, x = [0, 0, 1], [1, 0, 0]
    s, c = np.sin(0.5), np.cos(0.5)
    ps = np.zeros((5, 3), f32)
    pt = np.array([[6, 6, 7], [1, 0, 0], [1, 1e-20, 0], [-1, 1e-20, 0], [1, 0, 0]], f32)
    ns = np.array([z, [s, 0, c], x, x, x], f32)
    nt = np.array([z, [-s, 2.0, 0.25], z, z, z], f32)
    v, bins, pb = _check(host, ps, ns, pt, nt)
    assert pb["fragile"][[0, 2, 3]].all() and v[:2].all() and not v[4]
    assert bins[0, 2] in (8, 9) and bins[0, 0] == 5 and bins[0, 1] == 5
    assert (not v[2] or bins[2, 2] == 10) and (not v[3] or bins[3, 2] == 0)
    # duplicates whose float32 DistSq underflows to 0 although d != 0: invalid, as the contract counts in float32
    tiny = np.array([[1e-30, 0, 0]], f32)
    v, _ = run(host, np.zeros((1, 3), f32), [z], tiny, [z])
    assert v[0] == 0
