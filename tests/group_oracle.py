"""NumPy restatement of the group geometry contract (include/pcgx.h, "group geometry"; csrc/group_stats.hip).  No test
inside; tests/test_group_oracle.py checks it on hand-computed cases.

For a grouped id list over a tree's points (ids, sizes as pcgx_kdtree_clusters writes them):
  count, aabb   exact.
  centroid, cov the EXACT mean and covariance rounded once to float64: integer moments and fractions.Fraction
                (tests/cov_exact.py, imported and unchanged; its `one` calls a list of fewer than three neighbours
                degenerate, a covariance does not change when every member is taken three times, so it is).
  eig, axes     numpy.linalg.eigh of that covariance at unit trace, descending, the contract's signs, axis 2 = axis 0 x
                axis 1; trace 0: eig 0, axes identity.
  obb           the extents along those axes about that centroid in float64.
and the contract's bounds per group: D (the box diagonal), cov_bound = (2 n + 4) 2^-53 D^2, centroid_bound =
(n + 2) 2^-53 D + 2^-53 |c| per component."""
import collections
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_exact as CE  # noqa: E402

U53 = 2.0 ** -53
Stats = collections.namedtuple("Stats", "count aabb centroid cov eig axes obb")


def live(points, ids):
    """ids (m,) any ints -> bool (m,): 0 <= id < len(points) and the point's three coordinates finite"""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < len(P))
    ok[ok] = np.isfinite(P[ids[ok]]).all(axis=1)
    return ok


def slices(sizes, n_groups, cap_ids):
    """-> [(begin, end)] per group of [0, len(sizes)): the clamped sizes summed, clipped at cap_ids; groups >= n_groups own nothing"""
    out, at = [], 0
    for g, s in enumerate(np.asarray(sizes, np.int64)):
        s = max(int(s), 0) if g < n_groups else 0
        b, e = min(at, cap_ids), min(at + s, cap_ids)
        out.append((b, e))
        at += s
    return out


def sign(v):
    """the contract's sign: the component of largest magnitude positive, the first one on a tie"""
    v = np.array(v, np.float64)
    k = int(np.argmax(np.abs(v)))  # argmax returns the first maximum
    return -v if v[k] < 0 else v


def exact_mean(U, w):
    """the exact mean of the rows U (float32) taken w times each, rounded once"""
    ints, e = CE._integers(U.ravel())
    n = int(w.sum())
    return np.array([float(Fraction(sum(int(c) * v for c, v in zip(w, ints[a::3])), n) * Fraction(2) ** e) for a in range(3)])


def frame(cov6):
    """cov (6,) -> eig (3,) descending, axes (3, 3) rows, by numpy.linalg.eigh at unit trace"""
    tr = cov6[0] + cov6[3] + cov6[5]
    if not (tr > 0 and np.isfinite(tr)):
        return np.zeros(3), np.eye(3)
    lam, vec = np.linalg.eigh(CE.full(cov6) / tr)  # ascending, columns
    a0, a1 = sign(vec[:, 2]), sign(vec[:, 1])
    return lam[::-1] * tr, np.stack([a0, a1, np.cross(a0, a1)])


def obb(P, centroid, axes):
    e = (P.astype(np.float64) - centroid) @ axes.T  # (n, 3): (p - c) . axis_k
    lo, hi = e.min(axis=0), e.max(axis=0)
    return np.concatenate([centroid + ((hi + lo) / 2) @ axes, (hi - lo) / 2])


def group_stats(points, ids, sizes, n_groups=None, cap_ids=None):
    """points (n, 3) float32 (the tree's, deleted ones included); ids any ints; sizes (cap_groups,) ->
    (Stats over cap_groups rows, dict(D, cov_bound, centroid_bound, members: the live points per group))."""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    ids = np.asarray(ids, np.int64).reshape(-1)
    sizes = np.asarray(sizes, np.int64).reshape(-1)
    cap = len(sizes)
    G = cap if n_groups is None else min(max(int(n_groups), 0), cap)
    cap_ids = len(ids) if cap_ids is None else int(cap_ids)
    S = Stats(np.zeros(cap, np.int64), np.zeros((cap, 6), np.float32), np.zeros((cap, 3)), np.zeros((cap, 6)),
              np.zeros((cap, 3)), np.zeros((cap, 3, 3)), np.zeros((cap, 6)))
    info = dict(D=np.zeros(cap), cov_bound=np.zeros(cap), centroid_bound=np.zeros((cap, 3)), members=[None] * cap)
    for g, (b, e) in enumerate(slices(sizes, G, cap_ids)):
        m = ids[b:e]
        M = P[m[live(P, m)]]
        info["members"][g] = M
        n = len(M)
        if n == 0:
            continue
        S.count[g] = n
        S.aabb[g, :3], S.aabb[g, 3:] = M.min(axis=0), M.max(axis=0)
        U, w = np.unique(M, axis=0, return_counts=True)
        S.centroid[g] = exact_mean(U, w)
        S.cov[g] = CE.one(U, U[0], 3 * w)["cov6"]
        S.eig[g], S.axes[g] = frame(S.cov[g])
        S.obb[g] = obb(M, S.centroid[g], S.axes[g])
        D = float(np.linalg.norm(S.aabb[g, 3:].astype(np.float64) - S.aabb[g, :3].astype(np.float64)))
        info["D"][g] = D
        info["cov_bound"][g] = (2 * n + 4) * U53 * D * D
        info["centroid_bound"][g] = (n + 2) * U53 * D + U53 * np.abs(S.centroid[g])
    return S, info


def frame_residuals(cov6, eig, axes):
    """the two properties a frame is checked by, per group: max |axis_i . axis_j - delta_ij| and
    max_k ||cov axis_k - eig_k axis_k|| / trace (0 for a group of trace 0); both 0 for an all-zero row (a group without a
    live member) -> (orth (m,), eigres (m,))"""
    C = CE.full(np.asarray(cov6, np.float64).reshape(-1, 6))
    A = np.asarray(axes, np.float64).reshape(-1, 3, 3)
    E = np.asarray(eig, np.float64).reshape(-1, 3)
    orth = np.where(A.any(axis=(1, 2)), np.abs(A @ A.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2)), 0.0)
    tr = C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2]
    r = np.linalg.norm(A @ C - E[:, :, None] * A, axis=2).max(axis=1)  # rows: (C axis_k)^T = axis_k^T C
    return orth, np.where(tr > 0, r / np.where(tr > 0, tr, 1.0), 0.0)
