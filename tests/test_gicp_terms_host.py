"""csrc/gicp_terms.h compiled for the host with g++ (tests/cpp/gicp_terms_host.cpp over the shim
tests/cpp/host_shim), twice: -ffp-contract=off and -ffp-contract=fast with FMA instructions where the CPU has them.

Per pair against the NumPy oracle (tests/gicp_oracle.py) on three families: random SPD S, PLANE-mode S at
cond = 1 / eps, and the singular, indefinite and NaN cases (dropped, nothing written).

THE ENTRYWISE BOUND per term: c (kappa + 1) 2^-53 (|J|^T |M| |r|), kappa = cond_2(S).  c = 9 is the number of
roundings on the longest chain from the float32 inputs to a term in the expression as written; it is counted, step by
step, in the header's comment (an entry of M: 3, M r and M J_l: 6, a term: 9) and the header exports it as kGicpChain,
which this test reads back so the two cannot drift apart.  It is not fitted to the code's error.  One step of that
count is a CONVENTION, not a count: everything done in double-double arithmetic before the quotient (S, adjugate,
determinant, ~2^-104 relative per operation) stands for ONE rounding.  The worst observed share below is 0.88, so a
change to the dd_ helpers, or more dd operations, has to be looked at against this bound again.

The bound is entrywise, and H_01 = M_01 (likewise H_02, H_12) is a term on its own: an off-diagonal entry of S^-1 can
cancel to far below |M|'s scale, and a single float64 rounding of S moves it by 2^-53 (|M| |S| |M|)_kl, which
kappa |M_kl| does not bound.  An expression that factorises or inverts S in float64 therefore misses the bound on a
fraction of a per cent of random SPD pairs (a Cholesky form did: 178 of 50 000 at R = I, by up to 73 x), and so does a
float64 reference.  gicp_terms carries S, its adjugate and its determinant as sums of two float64 and rounds once, at
the quotient; the oracle (tests/gicp_oracle.py, pair_terms) works in numpy's extended precision.  Worst observed share
of the bound: random SPD S 0.15 at R = I and 0.88 at a 0.7 rad rotation; PLANE-mode S at cond = 1 / eps 6e-4.
THE NORMWISE BOUND (test_normwise_bound, every family, axis-aligned PLANE normals included, where M's off-diagonal
entries are rounding noise of the float32 covariances): c (kappa + 1) 2^-53 |M|_2 |J_k|_2 |r|_2 (|J_l|_2 for H) --
the same c and kappa with the entrywise products replaced by 2-norms (worst observed share 0.15)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gicp_oracle as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
C_CHAIN = 9
U = 2.0 ** -53


def _cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(" fma " in line + " " for line in f if line.startswith("flags"))
    except OSError:
        return False


VARIANTS = {"off": ["-ffp-contract=off"], "fast": ["-ffp-contract=fast"] + (["-mfma"] if _cpu_has_fma() else [])}


@pytest.fixture(scope="module", params=sorted(VARIANTS))
def host(request, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gicp_" + request.param) / "libgicp_terms_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC"]
                          + VARIANTS[request.param] +
                          ["-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "gicp_terms_host.cpp")])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run(lib, p, b, cb6, ct6, trans):
    p, b = np.ascontiguousarray(p, f32), np.ascontiguousarray(b, f32)
    cb6, ct6 = np.ascontiguousarray(cb6, f32), np.ascontiguousarray(ct6, f32)
    trans = np.ascontiguousarray(trans, f32)
    m = len(p)
    used = np.full(m, -1, np.int32)
    terms = np.full((m, 30), 7.25)  # (a sentinel: rows of dropped pairs must keep it)
    lib.gicp_terms_batch(_p(p), _p(b), _p(cb6), _p(ct6), _p(trans), ctypes.c_int64(m), _p(used), _p(terms))
    return used.astype(bool), terms


def _six(M):
    return np.stack([M[:, a, b] for a, b in G.UPPER], axis=1)


def _pose(rng, angle):
    """a rigid pose in float32, column-major"""
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = rng.standard_normal(3)
    return np.ascontiguousarray(T.T, f32).reshape(-1)


def _terms(lib, p, b, cb6, ct6, trans):
    cb6, ct6 = np.ascontiguousarray(cb6, f32), np.ascontiguousarray(ct6, f32)
    used, terms = run(lib, p, b, cb6, ct6, trans)
    o = G.pair_terms(p, b, G.cov_mats(cb6), G.cov_mats(ct6), G.rotation(trans))
    assert np.array_equal(used, o["used"])
    u = o["used"]
    assert np.all(terms[~u] == 7.25)
    assert np.all(terms[u][:, 28:] == 1.0)
    return used, terms, o


def _share(err, bound):
    over = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    return over.max() if over.size else 0.0, int((over.max(axis=1) > 1).sum()) if over.size else 0


def _check(lib, p, b, cb6, ct6, trans):
    """the entrywise bound"""
    used, terms, o = _terms(lib, p, b, cb6, ct6, trans)
    u = o["used"]
    bound = C_CHAIN * (o["kappa"][u, None] + 1) * U * o["absterms"][u]
    err = np.abs(terms[u] - o["terms"][u])
    share, over = _share(err, bound)
    print("entrywise bound: worst share %.3g, %d of %d pairs over (kappa up to %.3g)"
          % (share, over, int(u.sum()), np.nanmax(o["kappa"][u]) if u.any() else 0.0))
    assert np.all(err <= bound)
    return used


def _check_normwise(lib, p, b, cb6, ct6, trans):
    used, terms, o = _terms(lib, p, b, cb6, ct6, trans)
    u = o["used"]
    cb6, ct6 = np.ascontiguousarray(cb6, f32)[u], np.ascontiguousarray(ct6, f32)[u]
    R = G.rotation(trans)
    S = G.cov_mats(cb6) + R @ G.cov_mats(ct6) @ R.T
    mnorm = 1.0 / np.linalg.eigvalsh(S)[:, 0]  # |M|_2
    pd = np.asarray(p, f32)[u].astype(f64)
    rn = np.linalg.norm(pd - np.asarray(b, f32)[u].astype(f64), axis=1)
    jn = np.linalg.norm(G.jacobians(pd), axis=2)  # (m, 6)
    w = np.zeros((int(u.sum()), 30))
    w[:, 0] = rn * rn
    w[:, 1:7] = jn * rn[:, None]
    for n, (k, l) in enumerate(G.HKL):
        w[:, 7 + n] = jn[:, k] * jn[:, l]
    bound = C_CHAIN * (o["kappa"][u, None] + 1) * U * mnorm[:, None] * w
    err = np.abs(terms[u] - o["terms"][u])
    share, over = _share(err[:, :28], bound[:, :28])
    print("normwise bound: worst share %.3g (kappa up to %.3g)" % (share, np.nanmax(o["kappa"][u]) if u.any() else 0.0))
    assert np.all(err <= bound)
    return used


def _spd_family():
    rng = np.random.default_rng(1)
    m = 50_000
    A = rng.standard_normal((2, m, 3, 3))
    scale = 10.0 ** rng.uniform(-3, 1, (2, m, 1, 1))
    C = (A @ A.transpose(0, 1, 3, 2)) * scale + 1e-4 * scale * np.eye(3)
    p = (rng.standard_normal((m, 3)) * 5).astype(f32)
    b = p + (rng.standard_normal((m, 3)) * 0.1).astype(f32)
    return p, b, _six(C[0]), _six(C[1]), [_pose(rng, 0.0), _pose(rng, 0.7)]


def _plane_family(axis_aligned):
    """both covariances PLANE-mode about ONE shared normal (the target's is given in its own frame): cond(S) = 1 / eps"""
    rng = np.random.default_rng(2)
    m, eps = 50_000, 1e-3
    u = rng.standard_normal((m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    if axis_aligned:
        u[: m // 10] = np.eye(3)[rng.integers(0, 3, m // 10)]
    trans = _pose(rng, 0.3)
    R = G.rotation(trans)
    Cb = np.eye(3) - (1 - eps) * u[:, :, None] * u[:, None, :]
    ut = u @ R  # R ut = u
    Ct = np.eye(3) - (1 - eps) * ut[:, :, None] * ut[:, None, :]
    p = (rng.standard_normal((m, 3)) * 10).astype(f32)
    b = p + (rng.standard_normal((m, 3)) * 0.05).astype(f32)
    return p, b, _six(Cb), _six(Ct), trans, eps


def test_chain_constant_is_the_headers(host):
    assert host.gicp_chain() == C_CHAIN < 128


def test_random_spd(host):
    p, b, cb6, ct6, poses = _spd_family()
    for trans in poses:
        assert _check(host, p, b, cb6, ct6, trans).all()


def test_plane_mode_at_full_condition(host):
    p, b, cb6, ct6, trans, eps = _plane_family(axis_aligned=False)
    assert _check(host, p, b, cb6, ct6, trans).all()
    k = G.pair_terms(p, b, G.cov_mats(cb6.astype(f32)), G.cov_mats(ct6.astype(f32)), G.rotation(trans))["kappa"]
    assert np.median(k) > 0.9 / eps and k.max() < 1.1 / eps


def test_normwise_bound(host):
    p, b, cb6, ct6, poses = _spd_family()
    for trans in poses:
        assert _check_normwise(host, p, b, cb6, ct6, trans).all()
    p, b, cb6, ct6, trans, _ = _plane_family(axis_aligned=True)
    assert _check_normwise(host, p, b, cb6, ct6, trans).all()


def test_dropped_pairs_write_nothing(host):
    eye6 = np.array([1, 0, 0, 1, 0, 1], f64)
    flat = np.array([1, 0, 0, 1, 0, 0], f64)
    cases_b = [eye6 / 2, flat / 2, np.array([1, 0, 0, -3, 0, 1.0]), np.full(6, np.nan), np.zeros(6),
               np.array([1, 0, 0, 1, 0, np.nan]), -eye6, np.array([1, 2, 0, 1, 0, 1.0]), eye6 / 2]
    cases_t = [eye6 / 2, flat / 2, eye6, eye6, np.zeros(6), eye6, eye6 / 2, np.zeros(6),
               np.array([np.nan, 0, 0, 1, 0, 1])]
    m = len(cases_b)
    p, b = np.ones((m, 3), f32), np.zeros((m, 3), f32)
    ident = np.eye(4, dtype=f32).reshape(-1)
    used = _check(host, p, b, np.array(cases_b), np.array(cases_t), ident)
    assert used.tolist() == [True] + [False] * (m - 1)
    # RAW covariances of a lattice plane z = const under a rotation about z: S_zz == 0 exactly
    c, s = np.cos(0.3), np.sin(0.3)
    rot = np.eye(4)
    rot[:2, :2] = [[c, -s], [s, c]]
    used = _check(host, p, b, np.tile(flat, (m, 1)), np.tile(flat, (m, 1)), np.ascontiguousarray(rot.T, f32).reshape(-1))
    assert not used.any()
