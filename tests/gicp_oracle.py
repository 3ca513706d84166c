"""NumPy restatement of the Generalized ICP extension's contract (include/pcgx.h, "Generalized ICP").

NO REFERENCE PARITY EXISTS: pcgol has no GICP.  This file is the definition the tests hold the library to.  Pairs come
from the parity-pinned corresponder (oracle.KDTree.nearest_batch on synth.transform_points' float32 re-projection);
everything per pair is formed from the float32 inputs widened (in numpy's extended precision, rounded to float64 at
the end: the contract's float64 up to the reference's own error, which this keeps negligible):

    r = p - b,  S = C_b + R C_t R^T,  M = S^-1,  J_k = e_k,  J_{3+k} = e_k x p,
    e = r^T M r,  g_k = J_k^T M r,  H_kl = J_k^T M J_l (k <= l)

A pair is used only if S is positive definite by gauss_newton_solve's rule: trace(S) > 0 and every pivot of the
float64 Cholesky factorisation > 1e-12 trace(S).  The 30 sums are {sum e, sum g[6], upper triangle of sum H row-major
[21], sum w, pairs} with w = 1.  finish() and gauss_newton_update() restate pcgx_math.h with the roundings to float32
where the library has them: Evaluated's fields, d6, and the Mat4 / Rodrigues composition in float32."""
import os
import sys

import numpy as np

from pcgol_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

f32, f64, ld = np.float32, np.float64, np.longdouble
UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
P_VALUE, P_G0, P_H0, P_WEIGHT, P_PAIRS, P_COUNT = 0, 1, 7, 28, 29, 30
HKL = [(k, l) for k in range(6) for l in range(k, 6)]


class NotEnoughPairs(RuntimeError):
    pass


class Singular(RuntimeError):
    pass


def cov_mats(c6):
    """(n, 6) xx, xy, xz, yy, yz, zz float32 -> (n, 3, 3) float64"""
    c6 = np.asarray(c6, f32).reshape(-1, 6).astype(f64)
    C = np.empty((len(c6), 3, 3))
    for n, (a, b) in enumerate(UPPER):
        C[:, a, b] = c6[:, n]
        C[:, b, a] = c6[:, n]
    return C


def positive_definite(S):
    """The drop rule, vectorised: (m,) bool.  NaN fails the comparisons by itself."""
    with np.errstate(invalid="ignore", divide="ignore"):
        tr = (S[:, 0, 0] + S[:, 1, 1]) + S[:, 2, 2]
        tiny = tr * 1e-12
        ok = tr > 0.0
        s00 = S[:, 0, 0]
        ok &= s00 > tiny
        l00 = np.sqrt(np.where(ok, s00, 1.0))
        l10, l20 = S[:, 1, 0] / l00, S[:, 2, 0] / l00
        d1 = S[:, 1, 1] - l10 * l10
        ok &= d1 > tiny
        l11 = np.sqrt(np.where(ok, d1, 1.0))
        l21 = (S[:, 2, 1] - l20 * l10) / l11
        d2 = (S[:, 2, 2] - l20 * l20) - l21 * l21
        ok &= d2 > tiny
    return ok


def inverse3(S):
    """(m, 3, 3) symmetric -> S^-1 by the adjugate, in S's precision.  pair_terms works in numpy's extended precision
    (64-bit significand on x86: 2^-64 against float64's 2^-53), so that the reference's own error stays three orders
    below the bounds the tests hold the library to, also for an entry of S^-1 that nearly cancels."""
    a = np.empty_like(S)
    a[:, 0, 0] = S[:, 1, 1] * S[:, 2, 2] - S[:, 2, 1] * S[:, 2, 1]
    a[:, 0, 1] = a[:, 1, 0] = S[:, 2, 0] * S[:, 2, 1] - S[:, 1, 0] * S[:, 2, 2]
    a[:, 0, 2] = a[:, 2, 0] = S[:, 1, 0] * S[:, 2, 1] - S[:, 2, 0] * S[:, 1, 1]
    a[:, 1, 1] = S[:, 0, 0] * S[:, 2, 2] - S[:, 2, 0] * S[:, 2, 0]
    a[:, 1, 2] = a[:, 2, 1] = S[:, 1, 0] * S[:, 2, 0] - S[:, 0, 0] * S[:, 2, 1]
    a[:, 2, 2] = S[:, 0, 0] * S[:, 1, 1] - S[:, 1, 0] * S[:, 1, 0]
    det = S[:, 0, 0] * a[:, 0, 0] + S[:, 1, 0] * a[:, 0, 1] + S[:, 2, 0] * a[:, 0, 2]
    return a / det[:, None, None]


def jacobians(p):
    """(m, 3) float64 -> (m, 6, 3): J_k = e_k, J_{3+k} = e_k x p"""
    J = np.zeros((len(p), 6, 3), p.dtype)
    eye = np.eye(3, dtype=p.dtype)
    for k in range(3):
        J[:, k, :] = eye[k]
        J[:, 3 + k, :] = np.cross(np.broadcast_to(eye[k], p.shape), p)
    return J


def pair_terms(p, b, Cb, Ct, R):
    """p, b (m, 3) float32; Cb, Ct (m, 3, 3) float64; R (3, 3) float64 ->
    dict(used (m,) bool, terms (m, 30) [rows of unused pairs 0], absterms (m, 30): |J|^T |M| |r| and the like,
    kappa (m,) cond_2(S), NaN where unused)"""
    p = np.asarray(p, f32).astype(ld)
    b = np.asarray(b, f32).astype(ld)
    m = len(p)
    Rl = np.asarray(R).astype(ld)
    S = np.asarray(Cb).astype(ld) + Rl @ np.asarray(Ct).astype(ld) @ Rl.T
    used = positive_definite(S.astype(f64))
    terms, absterms, kappa = np.zeros((m, P_COUNT)), np.zeros((m, P_COUNT)), np.full(m, np.nan)
    u = np.nonzero(used)[0]
    if len(u):
        M = inverse3(S[u])
        r = (p - b)[u]
        J = jacobians(p[u])
        Mr = np.einsum("nab,nb->na", M, r)
        aMr = np.einsum("nab,nb->na", np.abs(M), np.abs(r))
        terms[u, P_VALUE] = np.einsum("na,na->n", r, Mr)
        absterms[u, P_VALUE] = np.einsum("na,na->n", np.abs(r), aMr)
        terms[u, P_G0:P_G0 + 6] = np.einsum("nka,na->nk", J, Mr)
        absterms[u, P_G0:P_G0 + 6] = np.einsum("nka,na->nk", np.abs(J), aMr)
        JM = np.einsum("nka,nab->nkb", J, M)
        aJM = np.einsum("nka,nab->nkb", np.abs(J), np.abs(M))
        for n, (k, l) in enumerate(HKL):
            terms[u, P_H0 + n] = np.einsum("nb,nb->n", JM[:, k], J[:, l])
            absterms[u, P_H0 + n] = np.einsum("nb,nb->n", aJM[:, k], np.abs(J[:, l]))
        terms[u, P_WEIGHT] = 1.0
        terms[u, P_PAIRS] = 1.0
        kappa[u] = np.linalg.cond(S[u].astype(f64))
    return dict(used=used, terms=terms, absterms=absterms, kappa=kappa)


def rotation(trans):
    return np.asarray(trans, f32).reshape(4, 4).T[:3, :3].astype(f64)  # column-major Mat4


def sums(tree, base_cov6, target, target_cov6, max_dist, trans=None):
    """One evaluation at pose `trans` (None: before the first update -- the target as it is, R = I).
    tree: oracle.KDTree (delete_point honoured).  -> dict(sums (30,), A (30,), kappa_max, dropped, used, matched)"""
    target = np.ascontiguousarray(target, f32).reshape(-1, 3)
    if trans is None:
        p, R = target, np.eye(3)
    else:
        p, R = synth.transform_points(np.asarray(trans, f32), target), rotation(trans)
    ids, _ = tree.nearest_batch(p, max_dist)
    has = np.nonzero(ids >= 0)[0]
    Cb = cov_mats(base_cov6)[ids[has]]
    Ct = cov_mats(target_cov6)[has]
    t = pair_terms(p[has], tree.pts[ids[has]], Cb, Ct, R)
    n_used = int(t["used"].sum())
    return dict(sums=t["terms"].sum(axis=0), A=t["absterms"].sum(axis=0),
                kappa_max=float(np.nanmax(t["kappa"])) if n_used else 0.0, dropped=len(has) - n_used, used=n_used,
                matched=len(has))


def finish(sums30, min_pairs=0):
    """finish_evaluate_plane (pcgx_math.h) behind the MinPairs test (0 -> 6)."""
    s = np.asarray(sums30, f64)
    if int(s[P_PAIRS]) < (min_pairs or 6):
        raise NotEnoughPairs(int(s[P_PAIRS]))
    sw = s[P_WEIGHT]
    f = 1.0 / sw if sw > 1.0 else 1.0
    H = np.zeros((6, 6), f32)
    for n, (k, l) in enumerate(HKL):
        H[k, l] = H[l, k] = f32(s[P_H0 + n] * (2.0 * f))
    return dict(value=f32(s[P_VALUE] * f), gradient=(s[P_G0:P_G0 + 6] * (2.0 * f)).astype(f32), hessian=H.reshape(-1),
                npairs=int(s[P_PAIRS]))


def _mat4_mul(m, a):
    """mat/mat4.go:16-28 in float32: out[4j+i] = sum_k m[4k+i] a[4j+k], accumulated from 0 in k order"""
    M, A = np.asarray(m, f32).reshape(4, 4).T, np.asarray(a, f32).reshape(4, 4).T  # [row, col]
    out = np.zeros((4, 4), f32)
    for k in range(4):
        out = out + np.outer(M[:, k], A[k, :]).astype(f32)  # float32 product, float32 addition
    return np.ascontiguousarray(out.T).reshape(-1)


def _translate(x, y, z):
    t = np.eye(4, dtype=f32).reshape(-1)
    t[12:15] = (x, y, z)
    return t


def _rodrigues(v):
    """icp/rodrigues.go:11-33 as pcgx_math.h restates it"""
    v = np.asarray(v, f32)
    ang = f32(np.sqrt(f64(f32(f32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))))
    r = np.zeros(16, f32)
    r[1], r[2], r[4], r[6], r[8], r[9] = v[2], -v[1], -v[2], v[0], v[1], -v[0]
    if ang < f32(0.1):
        f0, f1 = f32(1), f32(0.5)
    else:
        f0 = f32(f32(np.sin(f64(ang))) / ang)
        f1 = f32(f32(1.0 - np.cos(f64(ang))) / f32(ang * ang))
    ident = _translate(0, 0, 0)
    return ((ident + r * f0).astype(f32) + (_mat4_mul(r, r) * f1).astype(f32)).astype(f32)


def gauss_newton_solve(h36, g6, damping=0.0):
    a = np.asarray(h36, f32).reshape(6, 6).astype(f64)
    a[np.diag_indices(6)] += f64(f32(damping)) * np.diag(a)
    tr = np.trace(a)
    if not tr > 0.0:
        raise Singular()
    tiny = tr * 1e-12
    L = np.zeros((6, 6))
    for j in range(6):
        s = a[j, j] - np.dot(L[j, :j], L[j, :j])
        if not s > tiny:
            raise Singular()
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            L[i, j] = (a[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    y = np.linalg.solve(L, -np.asarray(g6, f32).astype(f64))
    return np.linalg.solve(L.T, y).astype(f32)


def gauss_newton_update(trans, it, ev, threshold=None, damping=0.0, max_iter=0):
    """-> (trans', converged, it'); raises Singular (trans unchanged)"""
    th = np.zeros(6, f32) if threshold is None else np.asarray(threshold, f32)
    if not np.any(th != 0):
        th = np.full(6, 0.01, f32)
    max_iter = max_iter or 20
    g = ev["gradient"]
    if not np.any((g < -th) | (th < g)):
        return np.asarray(trans, f32).copy(), True, it
    d = gauss_newton_solve(ev["hessian"], g, damping)
    trans = _mat4_mul(_translate(d[0], d[1], d[2]), _mat4_mul(_rodrigues(d[3:6]), trans))
    it += 1
    return trans, it >= max_iter, it


def fit(tree, base_cov6, target, target_cov6, max_dist, min_pairs=0, threshold=None, damping=0.0, max_iter=0,
        trace=None):
    """The Fit loop (icp.go:23-67 with the GICP evaluator and the Gauss-Newton updater).
    -> dict(trans, num_iteration, evaluated, dropped); trace: a list that receives every evaluation's sums() dict"""
    trans = _translate(0, 0, 0)
    it, num, ev, dropped = 0, 0, None, 0
    for _ in range(max_iter or 20):
        num += 1
        s = sums(tree, base_cov6, target, target_cov6, max_dist, trans if it > 0 else None)
        if trace is not None:
            trace.append(s)
        dropped = s["dropped"]
        ev = finish(s["sums"], min_pairs)
        trans, conv, it = gauss_newton_update(trans, it, ev, threshold, damping, max_iter)
        if conv:
            break
    return dict(trans=trans, num_iteration=num, evaluated=ev, dropped=dropped)


def knn_plane_covariances(points, k=20, eps=1e-3):
    """PLANE covariances of every point from a brute-force k-NN (tests/knn_oracle.py, tests/cov_oracle.py), float32."""
    import cov_oracle
    import knn_oracle
    ids, _, counts = knn_oracle.knearest(points, points, k, np.inf)
    return cov_oracle.covariances(points, points, ids, counts, cov_oracle.PLANE, eps)["cov6"].astype(f32)
