"""Self-checks of the Generalized ICP oracle (tests/gicp_oracle.py), the NumPy float64 restatement the GPU tests hold
the library to.  No GPU.

(a) C_b = C_t = I / 2 makes S = M = I: the sums are the point-to-point Gauss-Newton ones, e = |r|^2, g = J^T r.
(b) g is half the central finite difference of sum r^T M r over the six pose parameters, M frozen.
(c) the drop rule on singular, indefinite and NaN S.
(d) the Fit on synth.c4_plane(2500, width=1.5) with PLANE covariances (k = 20, eps = 1e-3) from a brute-force k-NN
    recovers inv(icp_pose()).  Measured here: |T - T_true|_max = 2.472e-07 after 6 iterations (MEASURED_FIT_ERROR) (a float64
    prototype of the contract reached 2.5e-8; this oracle rounds the pose to float32 as the library does).  The
    assertion is twice that plus 1e-6 for the float32 pose arithmetic."""
import os
import sys

import numpy as np

import oracle as O
from pcgol_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gicp_oracle as G  # noqa: E402

f32, f64 = np.float32, np.float64
MEASURED_FIT_ERROR = 2.5e-7  # (2.472e-07 measured)


def _scene(n=400, seed=3):
    rng = np.random.default_rng(seed)
    base = rng.random((n, 3)).astype(f32)
    target = synth.transform_points(synth.icp_pose(), base[rng.permutation(n)])
    return base, target


def _half_identity(n):
    return np.tile(np.array([0.5, 0, 0, 0.5, 0, 0.5], f32), (n, 1))


def test_identity_covariances_give_point_to_point_sums():
    base, target = _scene()
    tree = O.KDTree(base)
    for trans in (None, synth.icp_pose()):
        s = G.sums(tree, _half_identity(len(base)), target, _half_identity(len(target)), 0.5, trans)
        p = target if trans is None else synth.transform_points(trans, target)
        ids, _ = tree.nearest_batch(p, 0.5)
        has = ids >= 0
        pd, r = p[has].astype(f64), p[has].astype(f64) - base[ids[has]].astype(f64)
        J = G.jacobians(pd)
        # (R orthonormal to float32 only: S = I to ~1e-7, so the sums agree to that, not to the last bit)
        assert s["used"] == has.sum() and s["dropped"] == 0 and s["sums"][29] == s["sums"][28] == has.sum()
        assert np.isclose(s["sums"][0], np.sum(r * r), rtol=1e-6)
        assert np.allclose(s["sums"][1:7], np.einsum("nka,na->k", J, r), rtol=1e-6, atol=1e-6 * np.sum(np.abs(r)))
        H = np.einsum("nka,nla->kl", J, J)
        assert np.allclose(s["sums"][7:28], [H[k, l] for k, l in G.HKL], rtol=1e-6, atol=1e-6 * len(r))
        assert 1.0 <= s["kappa_max"] < 1.0 + 1e-5


def test_gradient_is_the_finite_difference_with_m_frozen():
    rng = np.random.default_rng(5)
    m = 300
    p, b = rng.random((m, 3)).astype(f32), rng.random((m, 3)).astype(f32)
    A = rng.standard_normal((2, m, 3, 3))
    Cb, Ct = A[0] @ A[0].transpose(0, 2, 1) + 0.1 * np.eye(3), A[1] @ A[1].transpose(0, 2, 1) + 0.1 * np.eye(3)
    R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    t = G.pair_terms(p, b, Cb, Ct, R)
    assert t["used"].all()
    M = np.linalg.inv(Cb + R @ Ct @ R.T)
    pd, bd = p.astype(f64), b.astype(f64)

    def cost(x):  # p' = p + t + w x p
        r = pd + x[:3] + np.cross(np.broadcast_to(x[3:], pd.shape), pd) - bd
        return np.einsum("na,nab,nb->", r, M, r)

    g = t["terms"][:, 1:7].sum(axis=0)
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        fd = (cost(d) - cost(-d)) / (2 * h)
        assert abs(fd - 2 * g[k]) <= 1e-7 * t["absterms"][:, 1 + k].sum()
    # H is the Gauss-Newton Hessian of the same cost: second difference (the cost is quadratic in x: exact up to rounding)
    Hs = t["terms"][:, 7:28].sum(axis=0)
    for n, (k, l) in enumerate(G.HKL):
        dk, dl = np.zeros(6), np.zeros(6)
        dk[k], dl[l] = 1e-3, 1e-3
        fd = (cost(dk + dl) - cost(dk - dl) - cost(dl - dk) + cost(-dk - dl)) / (4 * 1e-6)
        assert abs(fd - 2 * Hs[n]) <= 1e-6 * t["absterms"][:, 7 + n].sum()


def test_drop_rule():
    eye = np.eye(3)
    flat = np.diag([1.0, 1.0, 0.0])
    S = np.stack([eye, flat, np.diag([1.0, -1.0, 1.0]), np.full((3, 3), np.nan), np.zeros((3, 3)),
                  np.diag([1.0, 1.0, 1e-13]), np.diag([1.0, 1.0, 1e-11]), -eye,
                  np.array([[1.0, 2.0, 0], [2.0, 1.0, 0], [0, 0, 1.0]])])
    assert G.positive_definite(S).tolist() == [True, False, False, False, False, False, True, False, False]
    nan_entry = eye.copy()
    nan_entry[0, 1] = nan_entry[1, 0] = np.nan
    assert not G.positive_definite(nan_entry[None])[0]
    # through pair_terms: a dropped pair contributes nothing, to the pair count either
    p, b = np.ones((3, 3), f32), np.zeros((3, 3), f32)
    t = G.pair_terms(p, b, np.stack([eye / 2, flat / 2, np.full((3, 3), np.nan)]), np.stack([eye / 2, flat / 2, eye]), eye)
    assert t["used"].tolist() == [True, False, False]
    assert np.all(t["terms"][1:] == 0) and np.all(t["absterms"][1:] == 0) and t["terms"][0, 29] == 1
    assert np.isclose(t["terms"][0, 0], 3.0)


def test_plane_covariances_never_drop_and_bound_the_condition():
    rng = np.random.default_rng(9)
    m, eps = 20_000, 1e-3
    u = rng.standard_normal((2, m, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    C = np.eye(3) - (1 - eps) * u[..., :, None] * u[..., None, :]
    R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    S = C[0] + R @ C[1] @ R.T
    assert G.positive_definite(S).all()
    w = np.linalg.eigvalsh(S)
    assert w.min() >= 2 * eps * (1 - 1e-9) and w.max() <= 2 * (1 + 1e-9) and (w[:, 2] / w[:, 0]).max() <= (1 + 1e-9) / eps


def test_fit_recovers_the_pose_on_c4_plane():
    c = synth.c4_plane(2500, width=1.5)
    bc = G.knn_plane_covariances(c["base"])
    tc = G.knn_plane_covariances(c["target"])
    trace = []
    o = G.fit(O.KDTree(c["base"]), bc, c["target"], tc, c["max_dist"], 6, np.full(6, -1, f32), 0.0, 6, trace)
    inv = np.linalg.inv(synth.icp_pose().astype(f64).reshape(4, 4).T).T.reshape(-1)
    err = np.max(np.abs(o["trans"].astype(f64) - inv))
    print("gicp oracle fit: |T - T_true|_max = %.3e after %d iterations, dropped %d, kappa_max %.1f"
          % (err, o["num_iteration"], o["dropped"], trace[-1]["kappa_max"]))
    assert o["num_iteration"] == 6 and o["dropped"] == 0
    assert all(t["used"] == t["matched"] for t in trace) and trace[-1]["used"] > 0.99 * len(c["target"])
    assert err <= 2 * MEASURED_FIT_ERROR + 1e-6
    H = o["evaluated"]["hessian"].reshape(6, 6)
    assert np.array_equal(H, H.T) and np.all(np.diag(H) > 0)
