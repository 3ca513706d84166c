"""csrc/mls_terms.h compiled for the host with g++ (tests/cpp/mls_terms_host.cpp over the shim tests/cpp/host_shim),
twice: -ffp-contract=off and -ffp-contract=fast with FMA instructions where the CPU has them.

The frame, the sums of the normal equations, the 6 x 6 Cholesky and the finish -- the expressions the kernel compiles --
against the NumPy oracle (tests/mls_oracle.py) on 2000 random neighbourhoods of 6 to 200 points and on the hand cases
(tests/test_mls_oracle.py), with the tolerance and the bands the GPU tests use (mls_oracle.check): counts and kinds
exact off the fragile queries, positions within 2^-23 |x| + 1e-12 radius / pivot ratio, normals within sin 1e-6.  The
sums dealt out to several accumulators and merged (what a wave does with a fat row) pass the same checks."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mls_oracle as MO  # noqa: E402
import normals_oracle as NO  # noqa: E402
from test_fpfh_terms_host import VARIANTS  # noqa: E402
from test_mls_oracle import case_reference, check_case_kinds, hand_cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module", params=sorted(VARIANTS))
def host(request, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mls_" + request.param) / "libmls_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC"]
                          + VARIANTS[request.param] +
                          ["-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "mls_terms_host.cpp")])
    lib = ctypes.CDLL(so)
    lib.mls_pivot_min.restype = ctypes.c_double
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run(lib, points, queries, offs, ids, radius, sigma, order=2, min_neighbors=3, viewpoint=(0, 0, 0), parts=1):
    """-> ((points, normals, kinds, counts), pivot, c0) of the header over the given neighbour lists"""
    q = np.ascontiguousarray(queries, f32).reshape(-1, 3)
    nb = np.ascontiguousarray(np.asarray(points, f32).reshape(-1, 3)[ids])
    offs = np.ascontiguousarray(offs, np.int64)
    m = len(q)
    vp = np.asarray(viewpoint, f32)
    out_p, out_n = np.full((m, 3), -7, f32), np.full((m, 3), -7, f32)
    kinds, counts = np.full(m, -7, np.int32), np.full(m, -7, np.int32)
    pivot, c0 = np.full(m, -7, f64), np.full(m, -7, f64)
    lib.mls_terms_batch(_p(nb), _p(offs), _p(q), ctypes.c_int64(m), ctypes.c_float(radius), ctypes.c_float(sigma),
                        ctypes.c_int32(order), ctypes.c_int32(min_neighbors), _p(vp), ctypes.c_int32(parts), _p(out_p),
                        _p(out_n), _p(kinds), _p(counts), _p(pivot), _p(c0))
    return (out_p, out_n, kinds, counts), pivot, c0


def _random_neighbourhoods(m=2000, seed=11):
    """m patches of 6 to 200 points of a tilted, curved, noisy surface within the radius of a query near it"""
    rng = np.random.default_rng(seed)
    r = 0.15
    pts, offs, qs = [], [0], []
    for _ in range(m):
        k = int(rng.integers(6, 201))
        c = rng.uniform(-2, 2, 3)
        rot = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        rad = 0.95 * r * np.sqrt(rng.random(k))
        ang = rng.uniform(0, 2 * np.pi, k)
        x, y = rad * np.cos(ang), rad * np.sin(ang)
        kx, ky, kxy = rng.uniform(-2, 2, 3)
        z = 0.5 * kx * x * x + kxy * x * y + 0.5 * ky * y * y + 0.01 * rng.standard_normal(k)
        local = np.column_stack([x, y, z])
        pts.append((c + local @ rot.T).astype(f32))
        qs.append((c + np.array([0.0, 0.0, rng.uniform(-0.02, 0.02)]) @ rot.T).astype(f32))
        offs.append(offs[-1] + k)
    P = np.concatenate(pts)
    Q = np.array(qs, f32)
    # N(q) is what DistSq < r^2 says (float32), within each patch
    keep, new_offs = [], [0]
    for i in range(m):
        ids = np.arange(offs[i], offs[i + 1])
        ids = ids[NO.dist_sq_f32(P[ids], Q[i]) < f32(r) * f32(r)]
        keep.append(ids)
        new_offs.append(new_offs[-1] + len(ids))
    return P, Q, np.array(new_offs, np.int64), np.concatenate(keep), r


def test_constants_are_the_headers(host):
    assert host.mls_basis() == 6 and host.mls_sums() == 28
    assert host.mls_pivot_min() == MO.PIVOT_MIN


def test_random_neighbourhoods(host):
    P, Q, offs, ids, r = _random_neighbourhoods()
    counts = np.diff(offs)
    assert counts.min() <= 8 and counts.max() >= 190
    for order, sigma in ((2, r), (2, r / 2), (1, r)):
        ref = MO.mls_from_lists(P, Q, offs, ids, r, sigma, order, viewpoint=(0.5, 0.5, 9.0))
        for parts in (1, 64):
            got, pivot, c0 = run(host, P, Q, offs, ids, r, sigma, order, viewpoint=(0.5, 0.5, 9.0), parts=parts)
            g = MO.check(got, ref, r, "random order %d sigma %g parts %d" % (order, sigma, parts))
            if order == 2:
                assert g.sum() >= 0.9 * len(Q)
                # the header's own c0 is the oracle's where the solve is well conditioned (its sign is n's, which
                # either eigen-solver may return negated)
                assert np.all(np.abs(np.abs(c0[g]) - np.abs(ref["c0"][g])) <= 1e-12 * r / ref["pivot"][g])
            else:
                assert got[2].max() == 1 and np.all(pivot == 0.0)
                k1 = ref["kinds"] == 1  # the plane's projection: no solve, so no conditioning to divide by
                err = np.abs(got[0][k1].astype(f64) - ref["points"][k1].astype(f64))
                assert np.all(err <= 2.0 ** -23 * np.abs(ref["points"][k1].astype(f64)) + 1e-12 * r)


def test_hand_cases(host):
    for c in hand_cases():
        offs, ids = NO.brute_force_lists(c["points"], c["queries"], c["radius"])
        ref = case_reference(c)
        for parts in (1, 3):
            got, pivot, c0 = run(host, c["points"], c["queries"], offs, ids, c["radius"], c["sigma"], c["order"],
                                 c["min_neighbors"], parts=parts)
            points, normals, kinds, counts = got
            assert np.array_equal(counts, ref["counts"]), c["name"]
            check_case_kinds(c, kinds)
            z = kinds == 0
            assert np.array_equal(points[z].view(np.uint32), c["queries"][z].view(np.uint32)), c["name"]
            assert np.all(normals[z] == 0), c["name"]
            assert np.allclose(np.linalg.norm(normals[~z].astype(f64), axis=1), 1.0, atol=1e-6), c["name"]
            if not isinstance(c["kinds"], tuple):
                MO.check(got, ref, c["radius"], c["name"])
            if c["name"] == "coplanar lattice":
                assert np.all(np.abs(c0) <= 1e-12 * c["radius"])
                assert np.all(np.abs(normals.astype(f64) - [0, 0, -1]) <= 1e-7)
                assert np.all(np.abs(points[:, 2] - f32(0.5)) <= 2.0 ** -23)
            if c["name"].startswith("collinear"):
                assert np.max(np.abs(points.astype(f64) - c["queries"])) <= 1e-6 * c["radius"]


def test_nan_and_inf_queries(host):
    # (the neighbour lists are the caller's: an empty one is what DistSq < r^2 gives a NaN or an infinite query)
    lat = hand_cases()[7]["points"]
    q = f32([[np.nan, 0.25, 0.5], [np.inf, 0.25, 0.5]])
    got, _, _ = run(host, lat, q, np.zeros(3, np.int64), np.zeros(0, np.int64), 0.2, 0.2)
    assert got[2].tolist() == [0, 0] and got[3].tolist() == [0, 0]
    assert np.array_equal(got[0].view(np.uint32), q.view(np.uint32)) and np.all(got[1] == 0)
