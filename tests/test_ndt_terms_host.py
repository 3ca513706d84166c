"""csrc/ndt_terms.h compiled for the host with g++ (tests/cpp/ndt_terms_host.cpp over the shim tests/cpp/host_shim),
twice: -ffp-contract=off and -ffp-contract=fast with FMA instructions where the CPU has them.

The voxel finish, Magnusson's constants and one pair's terms -- the expressions the kernels compile -- against the
NumPy oracle (tests/ndt_oracle.py) on 3000 random voxels of 3 to 200 points, on the scenes of tests/test_ndt_oracle.py
(the hand cases among them) and on 4000 random pairs, with the tolerances the GPU tests use: voxels by
test_ndt_oracle.check_map, a pair's terms within kNdtChain 2^-53 of their sums of absolute values.  The voxels' sums
dealt out to 64 accumulators and merged (what a wave's lanes do) pass the same checks."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ndt_oracle as NO  # noqa: E402
from test_fpfh_terms_host import VARIANTS  # noqa: E402
from test_ndt_oracle import check_map, map_delta, map_scenes, scene_params  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module", params=sorted(VARIANTS))
def host(request, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ndt_" + request.param) / "libndt_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC"]
                          + VARIANTS[request.param] +
                          ["-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "ndt_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_voxels(lib, grid, pts, offs, v, min_points, ratio, parts=1):
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    offs = np.ascontiguousarray(offs, np.int64)
    v = np.ascontiguousarray(v, np.int64).reshape(-1, 3)
    m = len(v)
    origin = np.ascontiguousarray(grid.origin, f32)
    out = dict(count=np.full(m, -7, np.int32), valid=np.full(m, -7, np.int32), mean=np.full((m, 3), -7, f32),
               cov6=np.full((m, 6), -7, f32), icov6=np.full((m, 6), -7, f32))
    lib.ndt_voxels_batch(_p(pts), _p(offs), _p(v), ctypes.c_int64(m), _p(origin), ctypes.c_float(grid.resolution),
                         ctypes.c_int32(min_points), ctypes.c_float(ratio), ctypes.c_int32(parts), _p(out["count"]),
                         _p(out["valid"]), _p(out["mean"]), _p(out["cov6"]), _p(out["icov6"]))
    return out


def scene_lists(sc):
    """The buckets of a scene as the grid builds them: (points in bucket order, offsets, voxel coordinates)"""
    g, pts = sc["grid"], sc["base"]
    ok, _, a = g.addr(pts)
    ids = np.nonzero(ok)[0]
    order = ids[np.argsort(a[ids], kind="stable")]
    addrs, starts = np.unique(a[order], return_index=True)
    return pts[order], np.append(starts, len(order)), g.coords(addrs)


def _random_voxels(m=3000, seed=3):
    rng = np.random.default_rng(seed)
    grid = NO.Grid(0.5, (12, 12, 12), (-3.0, -3.0, -3.0))
    pts, offs, vs = [], [0], []
    for i in range(m):
        k = int(rng.integers(3, 201))
        v = rng.integers(0, 12, 3)
        rot = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        kind = i % 5   # blob, plate, needle, exact plane, exact line
        scale = [(0.1, 0.08, 0.05), (0.1, 0.08, 1e-3), (0.1, 1e-3, 5e-4), (0.1, 0.07, 0.0), (0.1, 0.0, 0.0)][kind]
        local = np.clip(rng.standard_normal((k, 3)) * scale, -0.13, 0.13)
        pts.append((grid.centre(v) + rng.uniform(-0.1, 0.1, 3) + local @ rot.T).astype(f32))
        offs.append(offs[-1] + k)
        vs.append(v)
    return grid, np.concatenate(pts), np.array(offs, np.int64), np.array(vs, np.int64)


def _oracle_voxels(grid, pts, offs, vs, min_points, ratio, parts=1):
    recs = [NO.voxel(pts[offs[i]:offs[i + 1]], grid.centre(vs[i]), min_points, ratio, parts) for i in range(len(vs))]
    m = len(recs)
    c64 = np.array([r["cov6"] for r in recs]).reshape(m, 6)
    i64 = np.array([r["icov6"] for r in recs]).reshape(m, 6)
    return dict(addr=np.arange(m), count=np.array([r["count"] for r in recs], np.int32),
                valid=np.array([r["valid"] for r in recs], np.int32), mean=np.array([r["mean"] for r in recs], f32),
                cov6_64=c64, icov6_64=i64)


def test_constants_are_the_headers(host):
    assert host.ndt_chain() == NO.CHAIN
    k2 = ctypes.c_double()
    for o, res in ((0.55, 0.5), (0.55, 1.0), (0.1, 0.25), (0.9, 2.0), (0.3, 0.05), (0.55, 10.0)):
        assert host.ndt_k2_host(ctypes.c_float(o), ctypes.c_float(res), ctypes.byref(k2)) == 1
        assert k2.value == NO.k2_of(o, res), (o, res)
    for o in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert host.ndt_k2_host(ctypes.c_float(o), ctypes.c_float(0.5), ctypes.byref(k2)) == 0
        assert NO.k2_of(o, 0.5) is None


def test_random_voxels(host):
    grid, pts, offs, vs = _random_voxels()
    ref = _oracle_voxels(grid, pts, offs, vs, 6, 0.01)
    dealt = _oracle_voxels(grid, pts, offs, vs, 6, 0.01, parts=64)
    v = ref["valid"] != 0
    assert 0.9 * len(vs) < v.sum() < len(vs)   # (voxels of 3 to 5 points are invalid)
    sens = max(float(np.max(np.abs(ref[k][v] - dealt[k][v]).max(axis=1) / np.abs(ref[k][v]).max(axis=1)))
               for k in ("cov6_64", "icov6_64"))
    delta = max(4.0 * sens, 64.0 / 0.01 * 2.0 ** -53)
    for parts in (1, 64):
        got = run_voxels(host, grid, pts, offs, vs, 6, 0.01, parts)
        got["addr"] = ref["addr"]
        check_map(got, ref, delta, "random voxels, parts %d" % parts)


def test_scenes_and_hand_cases(host):
    for name, sc in map_scenes().items():
        mp, ratio = scene_params(name)
        pts, offs, vs = scene_lists(sc)
        for parts in (1, 64):
            got = run_voxels(host, sc["grid"], pts, offs, vs, mp, ratio, parts)
            got["addr"] = sc["map"]["addr"]
            check_map(got, sc["map"], map_delta(name), "%s, parts %d" % (name, parts))
    # min_points below 3 counts as 3
    g = NO.Grid(1.0, (1, 1, 1), (0.0, 0.0, 0.0))
    two = run_voxels(host, g, f32([[0, 0, 0], [0.1, 0, 0]]), [0, 2], [[0, 0, 0]], 1, 0.01)
    three = run_voxels(host, g, f32([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]]), [0, 3], [[0, 0, 0]], -5, 0.01)
    assert two["valid"][0] == 0 and three["valid"][0] == 1


def test_random_pairs(host):
    rng = np.random.default_rng(4)
    sc = map_scenes()["prototype"]
    m = sc["map"]
    vi = np.nonzero(m["valid"])[0]
    n = 4000
    j = vi[rng.integers(0, len(vi), n)]
    spread = np.where(rng.random(n) < 0.2, 1.5, 0.2)[:, None]   # a fifth far away: omega underflows towards 0
    p = (m["mean"][j].astype(f64) + rng.standard_normal((n, 3)) * spread).astype(f32)
    k2 = NO.k2_of(0.55, 0.5)
    terms, absterms = NO.pair_terms(p, m["mean"][j], m["icov6"][j], k2)
    got = np.full((n, 30), -7.0)
    mean, icov = np.ascontiguousarray(m["mean"][j]), np.ascontiguousarray(m["icov6"][j])
    host.ndt_pairs_batch(_p(p), _p(mean), _p(icov), ctypes.c_int64(n), ctypes.c_double(k2), _p(got))
    err = np.abs(got - terms)
    # (an omega below 2^-1022 is a subnormal float64 and carries an absolute error of its own: 2^-1000 covers it)
    bound = NO.CHAIN * 2.0 ** -53 * absterms + 2.0 ** -1000
    assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(got[:, NO.P_PAIRS] == 1.0)
    w = got[:, NO.P_WEIGHT]
    assert w.min() < 1e-30 and w.max() > 0.5 and np.all(np.isfinite(got))
