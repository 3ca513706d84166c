"""csrc/group_terms.h compiled for the host with g++ -ffp-contract=off (tests/cpp/group_terms_host.cpp over the shim
tests/cpp/host_shim): the finish from given sums, the order of equal eigenvalues, the sign rule on ties, with +-0
components and a negative largest component, right-handed frames, the trace-0 and non-finite-trace branches, the
order-preserving keys -- and the measurement of the frame tolerance TAU of tests/test_gpu_group_stats.py: the residuals
of this host build and of numpy.linalg.eigh over that file's scenes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_oracle as GO  # noqa: E402
import group_scenes as GS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64

# The larger of the two residuals (orthonormality, eigen-equation over the trace) of the host-compiled group_terms.h and
# of numpy.linalg.eigh over the scenes of tests/group_scenes.py, as test_frame_residuals_on_the_scenes measures them
# (it prints the figures): 2.22e-15 (eigh's frames on the chain scene; the host
# build's own largest is 6.7e-16), rounded up.  tests/test_gpu_group_stats.py allows the device 4 x this.
TAU_MEASURED = 2.3e-15


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("group_terms") / "libgroup_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "group_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def frames(lib, cov6):
    cov6 = np.ascontiguousarray(cov6, f64).reshape(-1, 6)
    eig, axes = np.zeros((len(cov6), 3)), np.zeros((len(cov6), 3, 3))
    lib.group_frame_batch(_p(cov6), ctypes.c_int64(len(cov6)), _p(eig), _p(axes))
    return eig, axes


def host_stats(lib, pts, ids, sizes):
    """the whole call by the host build, live members only -> GO.Stats"""
    pts, ids = np.asarray(pts, f32), np.asarray(ids, np.int64)
    parts = [ids[b:e][GO.live(pts, ids[b:e])] for b, e in GO.slices(sizes, len(sizes), len(ids))]
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    P = np.ascontiguousarray(pts[np.concatenate(parts)] if len(parts) else np.zeros((0, 3), f32))
    g = len(sizes)
    S = GO.Stats(np.zeros(g, np.int64), np.zeros((g, 6), f32), np.zeros((g, 3)), np.zeros((g, 6)), np.zeros((g, 3)),
                 np.zeros((g, 3, 3)), np.zeros((g, 6)))
    lib.group_stats_host(_p(P), _p(offs), ctypes.c_int64(g), *[_p(a) for a in S])
    return S


def test_keys_f32(host):
    v = f32([-np.inf, -3.4028235e38, -1.0, -1.1754944e-38, -1e-45, -0.0, 0.0, 1e-45, 1.1754944e-38, 1.0, 3.4028235e38, np.inf])
    key, back = np.zeros(len(v), np.uint32), np.zeros(len(v), f32)
    host.group_keys_f32(_p(v), ctypes.c_int64(len(v)), _p(key), _p(back))
    assert np.array_equal(back.view(np.uint32), v.view(np.uint32))  # decoding gives the value back, -0 as -0
    for i in range(len(v)):
        for j in range(len(v)):
            if v[i] < v[j]:
                assert key[i] < key[j], (v[i], v[j])
    assert np.all(np.diff(key.astype(np.int64)) > 0)  # (-0 below +0: `<` calls them equal, a min may take either)
    assert key.max() < 0xFFFFFFFF and key.min() > 0  # the keys a min / a max starts from are outside


def test_keys_f64(host):
    v = f64([-np.inf, -1.7976931348623157e308, -1.0, -2.2250738585072014e-308, -5e-324, -0.0, 0.0, 5e-324,
             2.2250738585072014e-308, 1.0, 1.7976931348623157e308, np.inf])
    key, back = np.zeros(len(v), np.uint64), np.zeros(len(v), f64)
    host.group_keys_f64(_p(v), ctypes.c_int64(len(v)), _p(key), _p(back))
    assert np.array_equal(back.view(np.uint64), v.view(np.uint64))
    for i in range(len(v)):
        for j in range(len(v)):
            if v[i] < v[j]:
                assert int(key[i]) < int(key[j]), (v[i], v[j])
    assert all(int(a) < int(b) for a, b in zip(key[:-1], key[1:]))
    assert int(key.max()) < 2 ** 64 - 1 and int(key.min()) > 0


def test_live(host):
    xyz = f32([[0, 0, 0], [np.nan, 0, 0], [0, -np.inf, 0], [0, 0, np.inf], [1e-45, -3e38, 2]])
    for ids, want in (([0, 1, 2, 3, 4], [1, 0, 0, 0, 1]), ([-1, 5, 4, 0, 7], [0, 0, 0, 0, 0]), ([4, 4, 4, 4, 4], [1, 0, 0, 0, 1])):
        ids = np.array(ids, np.int64)
        out = np.full(5, -1, np.int32)
        host.group_live_batch(_p(ids), _p(xyz), ctypes.c_int64(5), ctypes.c_int64(5), _p(out))
        assert out.tolist() == want


def test_finish_from_given_sums(host):
    # four members at d = (+-1, +-2, 0) about the pivot (10, 20, 30), and the same sums shifted: d + (1, 0, 0)
    sums = f64([[0, 0, 0, 4, 0, 0, 16, 0, 0, 4], [4, 0, 0, 8, 0, 0, 16, 0, 0, 4], [3, 0, 0, 9, 0, 0, 0, 0, 0, 1]])
    pivot = f64([[10, 20, 30], [9, 20, 30], [-3, 1, 1]])
    cen, cov = np.zeros((3, 3)), np.zeros((3, 6))
    host.group_finish_batch(_p(sums), _p(pivot), ctypes.c_int64(3), _p(cen), _p(cov))
    assert cen.tolist() == [[10, 20, 30], [10, 20, 30], [0, 1, 1]]
    assert cov.tolist() == [[1, 0, 0, 4, 0, 0], [1, 0, 0, 4, 0, 0], [0, 0, 0, 0, 0, 0]]


def test_order_signs_and_degenerate_branches(host):
    inf, nan = np.inf, np.nan
    cov = f64([[1, 0, 0, 1, 0, 1],      # three equal eigenvalues: the order of the diagonal, identity
               [2, 0, 0, 5, 0, 2],      # y largest; x and z equal: x before z
               [3, 0, 0, 3, 0, 1],      # x and y equal and largest
               [1, 0, 0, 2, 0, 4],      # ascending on the diagonal
               [1, 1, 0, 1, 0, 0.5],    # eigenvectors (1, 1, 0) / sqrt 2 (2) and (1, -1, 0) / sqrt 2 (0): ties of magnitude
               [0, 0, 0, 0, 0, 0],      # trace 0
               [inf, 0, 0, 1, 0, 1],    # trace not finite
               [nan, 0, 0, 1, 0, 1],
               [-1, 0, 0, 0.5, 0, 0.25]])  # a trace that is not positive
    eig, axes = frames(host, cov)
    I = np.eye(3).tolist()
    assert eig[0].tolist() == [1, 1, 1] and axes[0].tolist() == I
    assert eig[1].tolist() == [5, 2, 2] and axes[1].tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, -1]]
    assert eig[2].tolist() == [3, 3, 1] and axes[2].tolist() == I
    assert eig[3].tolist() == [4, 2, 1] and axes[3].tolist() == [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]
    s = np.sqrt(0.5)
    assert np.allclose(eig[4], [2, 0.5, 0], atol=1e-15)
    assert np.allclose(axes[4], [[s, s, 0], [0, 0, 1], [s, -s, 0]], atol=1e-15)  # (s, -s, 0): the first of the tie is positive
    for k in (5, 6, 7, 8):
        assert eig[k].tolist() == [0, 0, 0] and axes[k].tolist() == I, k
    # the sign rule itself: ties, +-0 components, a negative largest component
    v = f64([[-0.6, 0.0, 0.8], [0.6, -0.0, -0.8], [-s, s, 0.0], [s, -s, -0.0], [0.0, -1.0, 0.0], [-0.0, 0.0, 1.0],
             [-0.5, -0.5, -s], [0.5, 0.5, -s - 1e-16]])
    w = v.copy()
    host.group_sign_batch(_p(w), ctypes.c_int64(len(w)))
    want = np.array([GO.sign(r) for r in v])
    assert np.array_equal(w, want)
    assert w[1].tolist() == [-0.6, 0.0, 0.8] and w[2].tolist() == [s, -s, -0.0] and w[4].tolist() == [-0.0, 1.0, -0.0]
    assert w[6].tolist() == [0.5, 0.5, s]


def test_random_frames_are_right_handed_and_match_eigh(host):
    rng = np.random.default_rng(3)
    Q = rng.normal(size=(2000, 3, 3))
    scale = 10.0 ** rng.uniform(-6, 6, (2000, 1, 1))
    M = Q @ Q.transpose(0, 2, 1) * scale
    M[:400] = (Q[:400, :, :1] @ Q[:400, :, :1].transpose(0, 2, 1)) * scale[:400]  # rank one: two zero eigenvalues
    cov6 = np.stack([M[:, a, b] for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)
    eig, axes = frames(host, cov6)
    tr = cov6[:, 0] + cov6[:, 3] + cov6[:, 5]
    assert np.all(np.diff(eig, axis=1) <= 0)
    assert np.allclose(np.linalg.det(axes), 1.0, atol=1e-14)
    orth, res = GO.frame_residuals(cov6, eig, axes)
    assert orth.max() <= 4 * TAU_MEASURED and res.max() <= 4 * TAU_MEASURED, (orth.max(), res.max())
    lam = np.linalg.eigvalsh(M / tr[:, None, None])[:, ::-1]
    assert np.abs(eig / tr[:, None] - lam).max() <= 4 * TAU_MEASURED
    for k in range(len(cov6)):  # the contract's signs
        for a in (0, 1):
            assert np.array_equal(GO.sign(axes[k, a]), axes[k, a])
        assert np.allclose(np.cross(axes[k, 0], axes[k, 1]), axes[k, 2], atol=0)


def _scenes():
    yield "boundaries", GS.boundaries()
    yield "boundaries reversed", GS.boundaries(reverse=True)
    yield "lattices", GS.lattices()[:3]
    yield "chain", GS.chain()
    yield "slots", GS.slots()


def test_frame_residuals_on_the_scenes(host):
    """TAU's measurement: over the device test's scenes, the residuals of the host build and of numpy.linalg.eigh (the
    oracle's frames on the exact covariance), the larger of the two <= TAU_MEASURED; and the host build against the
    oracle within the contract's bounds."""
    worst = 0.0
    for name, (pts, ids, sizes) in _scenes():
        want, info = GO.group_stats(pts, ids, sizes)
        got = host_stats(host, pts, ids, sizes)
        assert np.array_equal(got.count, want.count) and np.array_equal(got.aabb, want.aabb), name
        assert np.all(np.abs(got.cov - want.cov) <= info["cov_bound"][:, None]), name
        assert np.all(np.abs(got.centroid - want.centroid) <= info["centroid_bound"]), name
        figures = []
        for S in (got, want):
            orth, res = GO.frame_residuals(S.cov, S.eig, S.axes)
            figures += [orth.max(), res.max()]
        print("%s: host orth %.3g eig %.3g, eigh orth %.3g eig %.3g" % ((name,) + tuple(figures)))
        worst = max(worst, max(figures))
    print("largest residual %.3g" % worst)
    assert worst <= TAU_MEASURED
