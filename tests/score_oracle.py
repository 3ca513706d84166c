"""NumPy restatement of the contracts "score poses" and pcgx_pose_select (include/pcgx.h): brute force over every
(point, tree point) pair.  x' = pose_oracle.transform(pose, P), DistSq = (dx dx + dy dy) + dz dz in float32, the minimum
over the tree's points; a pair is found iff x' is finite and DistSq < max_dist^2.  A pair with DistSq == max_dist^2 is
"fragile": the library answers it by the reference's leaf / pivot rule, which this file does not restate -- it reports
such pairs, and the scenes (other than the boundary scene of tests/test_gpu_score_poses.py) must have none."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_oracle as PO  # noqa: E402

f32, f64 = np.float32, np.float64


def pose_live(pose):
    """a pose whose 16 numbers all compare equal to 0 is dead (a NaN compares unequal: live)"""
    return bool(np.any(~(np.asarray(pose, f32) == 0)))


def nearest_dist_sq(X, T, chunk=512):
    """X (n, 3), T (m, 3) float32 -> (n,) float32: the smallest DistSq from each row of X to a row of T (inf: m == 0)"""
    X, T = np.asarray(X, f32), np.asarray(T, f32)
    out = np.full(len(X), np.inf, f32)
    if len(T) == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(0, len(X), chunk):
            d = T[None, :, :] - X[i:i + chunk, None, :]
            out[i:i + chunk] = np.min((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], axis=1)
    return out


def score(T, P, poses, max_dist):
    """-> dict(counts int64 (K,), sums float64 (K,) by math.fsum, fragile int64 (K,), best, pose)"""
    poses = np.asarray(poses, f32).reshape(-1, 16)
    P = np.asarray(P, f32).reshape(-1, 3)
    md2 = f32(max_dist) * f32(max_dist)
    K = len(poses)
    counts, fragile, sums = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, f64)
    for k in range(K):
        if not pose_live(poses[k]) or len(P) == 0:
            continue
        x, y, z = PO.transform(poses[k], P)
        X = np.stack([x, y, z], axis=1)
        fin = np.isfinite(X).all(axis=1)
        d = np.full(len(P), np.inf, f32)
        if fin.any():
            d[fin] = nearest_dist_sq(X[fin], T)
        found = fin & (d < md2)
        counts[k] = int(found.sum())
        fragile[k] = int((fin & (d == md2)).sum())
        sums[k] = math.fsum(float(v) for v in d[found])
    live = [k for k in range(K) if pose_live(poses[k])]
    best = -1
    for k in live:  # the largest count, the smallest k among equals
        if best < 0 or counts[k] > counts[best]:
            best = k
    return dict(counts=counts, sums=sums, fragile=fragile, best=best, n_live=len(live),
                pose=poses[best].copy() if best >= 0 else np.zeros(16, f32))


def select(status, counts, poses, K):
    """-> (ids (K,) int64, poses (K, 16) float32, n_selected): status 0 and count >= 3, by count descending, then by h"""
    status, counts = np.asarray(status), np.asarray(counts, np.int64)
    poses = np.asarray(poses, f32).reshape(-1, 16)
    ok = [h for h in range(len(status)) if status[h] == 0 and counts[h] >= 3]
    ok.sort(key=lambda h: (-int(counts[h]), h))
    ok = ok[:K]
    ids = np.full(K, -1, np.int64)
    out = np.zeros((K, 16), f32)
    ids[:len(ok)] = ok
    if ok:
        out[:len(ok)] = poses[ok]
    return ids, out, len(ok)


def sum_bound(n, s):
    """|float64 sum of n non-negative terms in any order - the exact sum s| <= (n - 1) 2^-53 s (1 + ...); doubled"""
    return n * 2.0 ** -52 * s


# ---- the decoy scene: a wrong pose that collects more correspondences than the right one

DECOY_MAX_DIST, DECOY_EDGE = 0.02, 0.9
DECOY_TRIPLES = ((0, 6, 13), (14, 18, 23), (1, 7, 12), (15, 19, 22))


def _word_for(i, m):
    u = -((-i << 32) // m)  # the smallest sample word that names pair i of m (tests/test_pose_oracle.py, word_for)
    assert 0 <= u < 2 ** 32 and (u * m) >> 32 == i
    return u


@functools.lru_cache(maxsize=None)
def decoy_scene():
    """P against Q = P2 and 14 points of P under the decoy pose W: the true pose after a half turn of P about the
    vertical through c.  14 decoy pairs, 10 true pairs, two hypotheses from each kind.  Arrays are read-only."""
    P, P2 = PO.moved_clouds()
    R_true = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f64)
    t_true = np.array([2.25, -0.5, 1.75], f64)
    c = np.array([0.825, 0.825, 0.0], f64)
    Rz = np.diag([-1.0, -1.0, 1.0])
    t0 = c - Rz @ c
    W = PO.pose_mat(R_true @ Rz, R_true @ t0 + t_true)
    decoy_ids = 100 + 200 * np.arange(14)
    true_ids = 150 + 300 * np.arange(10)
    x, y, z = PO.transform(W, P[decoy_ids])
    Q = np.ascontiguousarray(np.concatenate([P2, np.stack([x, y, z], axis=1)]), f32)
    src = np.concatenate([decoy_ids, true_ids]).astype(np.int64)
    dst = np.concatenate([3000 + np.arange(14), true_ids]).astype(np.int64)
    m = len(src)
    samples = np.array([[_word_for(i, m) for i in row] for row in DECOY_TRIPLES], np.uint32)
    s = dict(P=P, P2=P2, Q=Q, W=W, src=src, dst=dst, pairs=np.stack([src, dst], axis=1), samples=samples,
             max_dist=DECOY_MAX_DIST, max_dist_sq=float(f32(DECOY_MAX_DIST) * f32(DECOY_MAX_DIST)), es=DECOY_EDGE)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def main_poses():
    """the six poses of the GPU tests' main scene: true, decoy, identity, true moved by 0.01, dead, one NaN entry"""
    s = decoy_scene()
    moved = PO.TRUE_POSE.copy()
    moved[12] += f32(0.01)
    nan = PO.TRUE_POSE.copy()
    nan[5] = np.nan
    return np.stack([PO.TRUE_POSE, s["W"], np.eye(4, dtype=f32).reshape(-1), moved, np.zeros(16, f32), nan]).astype(f32)
