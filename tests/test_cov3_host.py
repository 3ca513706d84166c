"""csrc/cov3.h compiled for the host with g++ (tests/cpp/cov3_host.cpp over the shim tests/cpp/host_shim), twice:
-ffp-contract=off and -ffp-contract=fast with FMA instructions where the CPU has them (the device build contracts).

The unit-trace Jacobi solve (norm_acc_solve) against numpy.linalg.eigh over random families and exact structured
matrices: Rayleigh excess u^T C u - lambda0 <= J tr, | |u| - 1 | <= 4 2^-53, the returned l0 within J of lambda0 / tr,
nothing NaN.  J = 32 2^-53: the backward-stability allowance of at most 24 plane rotations (8 sweeps of 3), each a
handful of float64 roundings on a unit-trace matrix; it is not fitted to the code.
The moments (NormAcc::add, norm_acc_cov) against the exact reference (tests/cov_exact.py): every entry within
B = (2 n + 4) 2^-53 S, from a query inside the list to one 1e6 away from a list 1e-3 wide; the far settings round the
trace to <= 0, the branch covariance_finish / normals_finish guard with `tr > 0.0`."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_exact as CE  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = 32 * 2.0 ** -53
N_RANDOM = 50_000


def _cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(" fma " in line + " " for line in f if line.startswith("flags"))
    except OSError:
        return False


VARIANTS = {"off": ["-ffp-contract=off"], "fast": ["-ffp-contract=fast"] + (["-mfma"] if _cpu_has_fma() else [])}


@pytest.fixture(scope="module", params=sorted(VARIANTS))
def host(request, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cov3_" + request.param) / "libcov3_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC"]
                          + VARIANTS[request.param] +
                          ["-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "cov3_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def solve(lib, c6):
    """-> (tr, l0, e (m,3), u (m,3)) with tr = xx + yy + zz in float64, as the kernels form it"""
    c6 = np.ascontiguousarray(c6, np.float64).reshape(-1, 6)
    tr = (c6[:, 0] + c6[:, 3]) + c6[:, 5]
    assert np.all(tr > 0)
    m = len(c6)
    l0, e, u = np.empty(m), np.empty((m, 3)), np.empty((m, 3))
    lib.cov3_solve(_p(c6), _p(tr), ctypes.c_int64(m), _p(l0), _p(e), _p(u))
    return tr, l0, e, u


def moments(lib, lists, q):
    """lists: (n_i, 3) float32 arrays, q (m, 3) float32 -> (c6 (m,6), tr (m,))"""
    offs = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(a) for a in lists], out=offs[1:])
    pts = np.ascontiguousarray(np.concatenate(lists), np.float32)
    q = np.ascontiguousarray(q, np.float32)
    c6, tr = np.empty((len(lists), 6)), np.empty(len(lists))
    lib.cov3_moments(_p(pts), _p(offs), _p(q), ctypes.c_int64(len(lists)), _p(c6), _p(tr))
    return c6, tr


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _six(M):
    return np.stack([M[:, a, b] for a, b in CE.UPPER], axis=1)


def _rotations(r, m):
    Qm, R = np.linalg.qr(r.normal(size=(m, 3, 3)))
    return Qm * np.sign(np.einsum("mii->mi", R))[:, None, :]


def _from_spectrum(r, lam):
    """V diag(lam) V^T with random rotations V, symmetrised"""
    V = _rotations(r, len(lam))
    M = np.einsum("mik,mk,mjk->mij", V, lam, V)
    return _six(0.5 * (M + M.transpose(0, 2, 1)))


def families(m=N_RANDOM):
    """name -> (m, 6): the lists a Jacobi solve goes wrong on"""
    r = _rng(7)
    u = lambda lo, hi, s: 10.0 ** r.uniform(lo, hi, s)  # noqa: E731
    f = {}
    f["generic"] = _from_spectrum(r, r.random((m, 3)) + 1e-3)
    f["planar"] = _from_spectrum(r, np.stack([u(-16, -6, m), r.random(m) + 0.1, r.random(m) + 0.1], 1))
    x = r.normal(size=(m, 3))
    f["rank1"] = _six(x[:, :, None] * x[:, None, :])
    l0 = r.random(m) * 0.1 + 1e-3
    f["l0~l1"] = _from_spectrum(r, np.stack([l0, l0 * (1.0 + u(-12, -3, m)), l0 + 1.0 + r.random(m)], 1))
    f["rod"] = _from_spectrum(r, np.stack([u(-12, -6, m), u(-12, -6, m), np.ones(m)], 1))
    f["isotropic"] = _from_spectrum(r, 1.0 + u(-15, -3, (m, 3)))
    f["scaled 1e+80"] = f["generic"] * 1e80
    f["scaled 1e-80"] = f["planar"] * 1e-80
    f["indefinite"] = _from_spectrum(r, np.stack([-u(-16, -2, m), r.random(m) * u(-16, 0, m), np.ones(m)], 1))
    f["float32 lattice"] = np.round(f["generic"] * 64.0) / 64.0 + np.float64([1, 0, 0, 1, 0, 1])
    return f


STRUCTURED = {
    "diag(1,0,0)": [1, 0, 0, 0, 0, 0], "diag(0,0,1)": [0, 0, 0, 0, 0, 1], "diag(0,1,0)": [0, 0, 0, 1, 0, 0],
    "diag(1,1,0)": [1, 0, 0, 1, 0, 0], "diag(0,1,1)": [0, 0, 0, 1, 0, 1], "diag(3,2,1)": [3, 0, 0, 2, 0, 1],
    "I": [1, 0, 0, 1, 0, 1], "all ones": [1, 1, 1, 1, 1, 1], "[[1,1,0],[1,1,0],[0,0,0]]": [1, 1, 0, 1, 0, 0],
    "[[0,0,0],[0,1,1],[0,1,1]]": [0, 0, 0, 1, 1, 1], "[[1,0,1],[0,0,0],[1,0,1]]": [1, 0, 1, 0, 0, 1],
    "circulant(2,-1,-1)": [2, -1, -1, 2, -1, 2], "circulant(2,1,1)": [2, 1, 1, 2, 1, 2],
    "I + tiny xy": [1, 1e-17, 0, 1, 0, 1], "I + tiny all": [1, 1e-19, -1e-19, 1, 1e-19, 1],
    "plane x+y+z": [2, -1, -1, 2, -1, 2], "plane x=y": [1, 1, 0, 1, 0, 4], "line (1,1,1)": [1, 1, 1, 1, 1, 1],
}


def solve_figures(lib, c6):
    """(Rayleigh excess / tr, | |u| - 1 |, |l0 - lambda0 / tr|, finite) per matrix, eigh on the unit-trace matrix"""
    tr, l0, e, u = solve(lib, c6)
    A = CE.full(c6) / tr[:, None, None]
    lam = np.linalg.eigvalsh(A)
    ray = np.einsum("mi,mij,mj->m", u, A, u) - lam[:, 0]
    finite = np.isfinite(l0) & np.isfinite(e).all(1) & np.isfinite(u).all(1)
    return ray, np.abs(np.linalg.norm(u, axis=1) - 1.0), np.abs(l0 - lam[:, 0]), finite


def test_solve_against_eigh(host):
    cases = dict(families())
    cases["structured"] = np.float64(list(STRUCTURED.values()))
    worst = {}
    for name, c6 in cases.items():
        ray, unit, dl, finite = solve_figures(host, c6)
        worst[name] = (float(ray.max()), float(unit.max()), float(dl.max()), bool(finite.all()))
        print("%-16s Rayleigh excess %.2e (%.2f J)  | |u| - 1 | %.2e  |l0 - lambda0| %.2e (%.2f J)"
              % (name, ray.max(), ray.max() / J, unit.max(), dl.max(), dl.max() / J))
    for name, (ray, unit, dl, finite) in worst.items():
        assert finite, name
        assert ray <= J, (name, ray)
        assert unit <= 4 * 2.0 ** -53, (name, unit)
        assert dl <= J, (name, dl)


def test_structured_matrices_exactly(host):
    """where the answer is known in closed form: the eigenvalue, and the eigenvector where it is unique"""
    s = np.sqrt
    want = {"diag(1,0,0)": (0.0, None), "diag(0,0,1)": (0.0, None), "diag(1,1,0)": (0.0, [0, 0, 1]),
            "diag(0,1,1)": (0.0, [1, 0, 0]), "diag(3,2,1)": (1 / 6, [0, 0, 1]), "I": (1 / 3, None),
            "all ones": (0.0, None), "[[1,1,0],[1,1,0],[0,0,0]]": (0.0, None),
            "circulant(2,-1,-1)": (0.0, [1 / s(3), 1 / s(3), 1 / s(3)]), "circulant(2,1,1)": (1 / 6, None),
            "plane x=y": (0.0, [1 / s(2), -1 / s(2), 0])}
    for name, (lam0, vec) in want.items():
        _, l0, e, u = solve(host, np.float64([STRUCTURED[name]]))
        assert abs(l0[0] - lam0) <= J, (name, l0[0])
        assert abs(e[0].sum() - 1.0) <= J, name
        if vec is not None:
            assert abs(abs(u[0] @ np.float64(vec)) - 1.0) <= J, (name, u[0])


SETTINGS = ((0.1, 0.0), (0.1, 10.0), (1e-3, 1e3), (2e-7, 1e2), (2e-7, 1e4), (1e-3, 1e6))


def far_lists(r, spread, dist, m):
    """m lists of 3..64 float32 points within `spread` of (1, 1, 1), each with a query `dist` away"""
    lists, qs = [], []
    for _ in range(m):
        n = int(r.integers(3, 65))
        lists.append((1.0 + spread * r.uniform(-1, 1, (n, 3))).astype(np.float32))
        d = r.normal(size=3)
        qs.append((1.0 + dist * d / np.linalg.norm(d)).astype(np.float32))
    return lists, np.float32(qs)


def test_moments_within_the_forward_bound(host):
    r = _rng(11)
    cancelled = {}
    for spread, dist in SETTINGS:
        lists, q = far_lists(r, spread, dist, 200)
        c6, tr = moments(host, lists, q)
        worst, n_exact = 0.0, 0
        for i, P in enumerate(lists):
            e = CE.one(P, q[i])
            if e["S"] == 0.0:
                continue
            err = np.abs(c6[i] - e["cov6"])
            assert np.all(err <= e["B"]), (spread, dist, i, err / e["B"])
            assert abs(tr[i] - e["trace"]) <= 3 * e["B"], (spread, dist, i)
            worst = max(worst, float(err.max() / e["B"]))
            n_exact += 1
        cancelled[(spread, dist)] = int((tr <= 0).sum())
        print("spread %g, query %g away: worst |C - C_exact| = %.3f B over %d lists, tr <= 0 in %d"
              % (spread, dist, worst, n_exact, cancelled[(spread, dist)]))
        assert np.isfinite(c6).all()
    assert cancelled[(0.1, 0.0)] == 0 and cancelled[(0.1, 10.0)] == 0 and cancelled[(1e-3, 1e3)] == 0
    assert max(cancelled.values()) > 0  # the guarded branch is reachable with plain float32 input


def test_moments_on_exact_lattices(host):
    """lists whose float64 moments are exact (small integers over a power of two, n a power of two): bit for bit the
    exact C, whatever the contraction; the trace of a single place is 0 exactly"""
    r = _rng(12)
    lists = [(r.integers(0, 16, (n, 3)) / 16.0).astype(np.float32) for n in (4, 8, 16, 32, 64) for _ in range(20)]
    lists += [np.tile(np.float32([[0.5, 0.25, 0.75]]), (8, 1))]
    q = np.float32([r.integers(0, 16, 3) / 16.0 for _ in lists])
    c6, tr = moments(host, lists, q)
    for i, P in enumerate(lists):
        e = CE.one(P, q[i])
        assert np.array_equal(c6[i], e["cov6"]) and tr[i] == e["trace"], i
    assert tr[-1] == 0.0
