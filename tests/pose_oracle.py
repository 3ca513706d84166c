"""NumPy restatement of the contract "pose from correspondences" (include/pcgx.h): what pcgx_pose_from_correspondences
must compute.  Statuses, counts, the first best and the inlier lists are exact; the rigid solve is an independent method
(Kabsch: numpy.linalg.svd with the determinant correction, float64), so poses are compared within the bound of
POSE_TOL on well-conditioned triangles (sin^2 >= WELL)."""
import numpy as np

f32, f64, u32 = np.float32, np.float64, np.uint32
OK, BAD_SAMPLE, DEGENERATE, EDGE = 0, 1, 2, 3
TRIANGLE_EPS = 1e-12
REFIT_GAP = 1e-9
WELL = 1e-4            # sin^2 of a triangle's angle at x0 below which the pose comparison leaves a hypothesis out
POSE_TOL = 2.0 ** -23  # * max(1, |oracle's|): one float32 rounding (2^-24 relative), a factor two for the float64 solve


def sample_index(u, m):
    return ((np.asarray(u, np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def _norm_sq(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def triangle_terms(X):
    """X (..., 3, 3) float32 triangles -> (|e1 x e2|^2, |e1|^2, |e2|^2) in float64"""
    X = np.asarray(X, f32).astype(f64)
    e1, e2 = X[..., 1, :] - X[..., 0, :], X[..., 2, :] - X[..., 0, :]
    return _norm_sq(_cross(e1, e2)), _norm_sq(e1), _norm_sq(e2)


def triangle_degenerate(X):
    with np.errstate(invalid="ignore", over="ignore"):
        c2, a2, b2 = triangle_terms(X)
        return ~(c2 > (TRIANGLE_EPS * a2) * b2)


def sin_sq(X):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c2, a2, b2 = triangle_terms(X)
        return c2 / (a2 * b2)


def edges_differ(P3, Q3, s):
    """P3, Q3 (..., 3, 3) float32; s: edge_similarity, a float32 value"""
    P3, Q3 = np.asarray(P3, f32).astype(f64), np.asarray(Q3, f32).astype(f64)
    s = f64(f32(s))
    ok = np.ones(P3.shape[:-2], bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, j in ((0, 1), (0, 2), (1, 2)):
            ls = np.sqrt(_norm_sq(P3[..., j, :] - P3[..., i, :]))
            ld = np.sqrt(_norm_sq(Q3[..., j, :] - Q3[..., i, :]))
            ok &= (ls >= s * ld) & (ld >= s * ls)
    return ~ok


def kabsch(P, Q):
    """the proper rotation R and translation t minimising sum |R p + t - q|^2 over the rows of P, Q (float64), and the
    singular values / determinant sign the refit's degeneracy rule is stated in"""
    P, Q = np.asarray(P, f32).astype(f64), np.asarray(Q, f32).astype(f64)
    cp, cq = P.mean(axis=0), Q.mean(axis=0)
    H = (P - cp).T @ (Q - cq)  # sum p q^T, centred
    U, S, Vt = np.linalg.svd(H)
    d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, cq - R @ cp, S, d


def pose_mat(R, t):
    """column-major float32 4 x 4, each number rounded once"""
    m = np.zeros(16, f32)
    for c in range(3):
        m[4 * c:4 * c + 3] = R[:, c].astype(f32)
    m[12:15] = np.asarray(t).astype(f32)
    m[15] = 1.0
    return m


def transform(pose, P):
    """mat4_transform as pcgx_math.h writes it, float32, nothing fused; pose (..., 16) against P (n, 3) broadcasts to
    (..., n)"""
    m = np.asarray(pose, f32)[..., None]
    P = np.asarray(P, f32)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = f32(1.0) / (((m[..., 3, :] * x + m[..., 7, :] * y) + m[..., 11, :] * z) + m[..., 15, :])
        ox = (((m[..., 0, :] * x + m[..., 4, :] * y) + m[..., 8, :] * z) + m[..., 12, :]) * w
        oy = (((m[..., 1, :] * x + m[..., 5, :] * y) + m[..., 9, :] * z) + m[..., 13, :]) * w
        oz = (((m[..., 2, :] * x + m[..., 6, :] * y) + m[..., 10, :] * z) + m[..., 14, :]) * w
    return ox, oy, oz


def dist_sq(pose, P, Q):
    ox, oy, oz = transform(pose, P)
    Q = np.asarray(Q, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = Q[:, 0] - ox, Q[:, 1] - oy, Q[:, 2] - oz
        return (dx * dx + dy * dy) + dz * dz


def pair_points(P, Q, src, dst):
    """the pairs' points, NaN where an id is out of range (never an inlier), and which pairs are in range"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    ok = (src >= 0) & (src < len(P)) & (dst >= 0) & (dst < len(Q))
    A = np.full((len(src), 3), np.nan, f32)
    B = np.full((len(src), 3), np.nan, f32)
    A[ok] = np.asarray(P, f32)[src[ok]]
    B[ok] = np.asarray(Q, f32)[dst[ok]]
    return A, B, ok


def inlier_mask(pose, A, B, max_dist_sq):
    """pose (..., 16) -> (..., m) bool"""
    with np.errstate(invalid="ignore"):
        return dist_sq(pose, A, B) < f32(max_dist_sq)


def count_under(poses, A, B, max_dist_sq, chunk=256):
    poses = np.asarray(poses, f32).reshape(-1, 16)
    out = np.zeros(len(poses), np.int64)
    for i in range(0, len(poses), chunk):
        out[i:i + chunk] = inlier_mask(poses[i:i + chunk], A, B, max_dist_sq).sum(axis=1)
    return out


def hypotheses(P, Q, src, dst, samples, edge_similarity):
    """-> status (n_hyp,) int32, poses (n_hyp, 16) float32, idx (n_hyp, 3) the sampled pairs"""
    samples = np.asarray(samples, u32).reshape(-1, 3)
    n, m = len(samples), len(src)
    status = np.full(n, BAD_SAMPLE, np.int32)
    poses = np.zeros((n, 16), f32)
    if m < 3:
        return status, poses, np.zeros((n, 3), np.int64)
    idx = sample_index(samples, m)
    A, B, ok = pair_points(P, Q, src, dst)
    good = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2]) & ok[idx].all(axis=1)
    P3, Q3 = A[idx], B[idx]
    deg = triangle_degenerate(P3) | triangle_degenerate(Q3)
    edge = edges_differ(P3, Q3, edge_similarity) if f32(edge_similarity) > 0 else np.zeros(n, bool)
    status[good & deg] = DEGENERATE
    status[good & ~deg & edge] = EDGE
    status[good & ~deg & ~edge] = OK
    for h in np.nonzero(status == OK)[0]:
        R, t, _, _ = kabsch(P3[h], Q3[h])
        poses[h] = pose_mat(R, t)
    return status, poses, idx


def well_conditioned(P, Q, src, dst, idx):
    A, B, _ = pair_points(P, Q, src, dst)
    with np.errstate(invalid="ignore"):
        return (sin_sq(A[idx]) >= WELL) & (sin_sq(B[idx]) >= WELL)


def first_best(status, counts):
    """-> (best, best_count, found): the status-0 hypothesis with the largest count, the smallest h among equals"""
    okh = np.nonzero(np.asarray(status) == OK)[0]
    if len(okh) == 0:
        return -1, 0, False
    c = np.asarray(counts)[okh]
    best = int(okh[int(np.argmax(c))])  # (argmax returns the first maximum)
    return best, int(c.max()), bool(c.max() >= 3)


def refit(A, B, ids):
    """the refined pose over the pairs `ids`, or None where the set is too degenerate to refit"""
    if len(ids) < 3:
        return None
    R, t, S, d = kabsch(A[ids], B[ids])
    l1, gap = S[0] + S[1] + d * S[2], 2.0 * (S[1] + d * S[2])
    if not (gap > REFIT_GAP * l1):
        return None
    return pose_mat(R, t)


def pose_close(got, want):
    """every one of the twelve numbers within POSE_TOL * max(1, |want|); -> (ok, the largest difference over its bound)"""
    got, want = np.asarray(got, f32).astype(f64), np.asarray(want, f32).astype(f64)
    r = np.abs(got - want) / (POSE_TOL * np.maximum(1.0, np.abs(want)))
    return bool(np.all(r <= 1.0)), float(r.max()) if r.size else 0.0


def estimate(P, Q, src, dst, samples, max_dist_sq, edge_similarity, refine, poses=None):
    """The whole call.  `poses`: take these bits (the library's) for the hypotheses instead of the oracle's own solve,
    so that counts, the best and the lists can be compared exactly."""
    status, own, idx = hypotheses(P, Q, src, dst, samples, edge_similarity)
    poses = own if poses is None else np.asarray(poses, f32).reshape(-1, 16)
    A, B, _ = pair_points(P, Q, src, dst)
    m = len(src)
    counts = np.where(status == OK, count_under(poses, A, B, max_dist_sq), 0) if m else np.zeros(len(status), np.int64)
    best, best_count, found = first_best(status, counts)
    out = dict(status=status, poses=poses, own_poses=own, idx=idx, counts=counts, best=best, best_count=best_count,
               found=found, refined=False, pose=np.zeros(16, f32), inliers=np.zeros(0, np.int64), refit_pose=None)
    if best < 0:
        return out
    out["pose"] = poses[best].copy()
    out["inliers"] = out["best_inliers"] = np.nonzero(inlier_mask(poses[best], A, B, max_dist_sq))[0]
    if refine and found:
        r = refit(A, B, out["inliers"])
        out["refit_pose"] = r
        if r is not None:
            ids2 = np.nonzero(inlier_mask(r, A, B, max_dist_sq))[0]
            if len(ids2) >= best_count:
                out.update(refined=True, pose=r, inliers=ids2)
    return out


# ---- scene M: the moved clouds of tests/test_gpu_match.py (the recipe, copied), 1500 pairs of which 40 % are redrawn

def moved_clouds():
    rng = np.random.default_rng(77)
    xy = rng.integers(0, 1690, (3000, 2)).astype(f64) / 1024.0
    x, y = xy[:, 0], xy[:, 1]
    z = np.rint((0.5 * np.sin(0.7 * x) * np.cos(0.5 * y) + 0.3 * np.sin(1.3 * y)) * 1024.0) / 1024.0
    P = np.ascontiguousarray(np.stack([x, y, z], axis=1), f32)
    P2 = np.ascontiguousarray(np.stack([-P[:, 1], P[:, 0], P[:, 2]], axis=1) + np.array([2.25, -0.5, 1.75], f32), f32)
    return P, P2


TRUE_POSE = np.array([0, 1, 0, 0, -1, 0, 0, 0, 0, 0, 1, 0, 2.25, -0.5, 1.75, 1], f32)  # column-major


def scene_m():
    P, P2 = moved_clouds()
    rng = np.random.default_rng(5)
    src = np.sort(rng.choice(3000, 1500, replace=False)).astype(np.int64)
    dst = src.copy()
    wrong = rng.random(1500) < 0.4
    dst[wrong] = rng.integers(0, 3000, int(wrong.sum()))
    samples = np.random.default_rng(11).integers(0, 2 ** 32, (4096, 3)).astype(u32)
    return dict(P=P, Q=P2, src=src, dst=dst, samples=samples, max_dist=0.01, max_dist_sq=float(f32(0.01) * f32(0.01)))
