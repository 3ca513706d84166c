"""The contract of pcgx_kdtree_planes (include/pcgx.h, "planes") restated in NumPy: the live points, the rounds, the
hypotheses' status and plane (float64, one rounding an operation), the strict float32 inlier test, the first best, the
refinement rule and the outputs.  `segment` takes `hyp_planes=` so that counts can be checked at the library's own plane
bits, and `group_stats=` -- the least-squares frame of an id list: the library's KDTree.GroupStats on the GPU (device
against device; GroupStats is pinned to its own oracle), or `lstsq_frame` below, an eigh restatement that is NOT bit-exact
and serves the CPU tests of the rules."""
import collections

import numpy as np

f32, f64 = np.float32, np.float64
NOT_RUN, OK, BAD_SAMPLE, DEGENERATE, AXIS = -1, 0, 1, 2, 3
TRIANGLE_EPS = 1e-12

Result = collections.namedtuple("Result", "n_planes planes sizes refined best labels ids status counts hyp_planes "
                                          "pre_ids")  # pre_ids: per found round, the best hypothesis's inliers


def sample_index(u, m):
    return (int(u) * int(m)) >> 32


def triangle_degenerate(x0, x1, x2):
    x0, x1, x2 = (np.asarray(v, f32).astype(f64) for v in (x0, x1, x2))
    with np.errstate(all="ignore"):
        a, b = x1 - x0, x2 - x0
        c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        c2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        a2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
        b2 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
        return not bool(c2 > (TRIANGLE_EPS * a2) * b2)


class Axis:
    """The axis constraint: a (float64 from float32), |a| = sqrt((ax ax + ay ay) + az az), the bound as float64."""

    def __init__(self, axis, min_axis_cos):
        self.a = np.asarray(axis, f32).astype(f64).reshape(3)
        a = self.a
        self.norm = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
        self.cos = f64(f32(min_axis_cos))

    def dot(self, n):
        return (n[0] * self.a[0] + n[1] * self.a[1]) + n[2] * self.a[2]


def axis_ok(n, A):
    return A is None or bool(abs(A.dot(n)) >= A.cos * A.norm)


def orient(n, A):
    s = A.dot(n) if A is not None else 0.0
    if A is not None and s != 0.0:
        flip = s < 0.0
    else:
        m = np.abs(n)
        lead = n[0] if (m[0] >= m[1] and m[0] >= m[2]) else (n[1] if m[1] >= m[2] else n[2])
        flip = lead < 0.0
    return -n if flip else n


def _plane(n, p):
    d = -((n[0] * p[0] + n[1] * p[1]) + n[2] * p[2])
    return np.array([n[0], n[1], n[2], d], f64).astype(f32)


def hypothesis(i0, i1, i2, p0, p1, p2, A=None):
    """-> (status, plane float32 (4,)): the plane through three points at the indices i0, i1, i2."""
    zero = np.zeros(4, f32)
    if i0 == i1 or i0 == i2 or i1 == i2:
        return BAD_SAMPLE, zero
    if triangle_degenerate(p0, p1, p2):
        return DEGENERATE, zero
    p0, p1, p2 = (np.asarray(v, f32).astype(f64) for v in (p0, p1, p2))
    a, b = p1 - p0, p2 - p0
    c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    n = c / np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    if not axis_ok(n, A):
        return AXIS, zero
    return OK, _plane(orient(n, A), p0)


def refit(centroid, axis2, eig0, A=None):
    """-> (ok, plane): the refitted plane from group geometry's centroid, axis 2 and largest eigenvalue."""
    if not eig0 > 0.0:
        return False, np.zeros(4, f32)
    n = np.asarray(axis2, f64).copy()
    if not axis_ok(n, A):
        return False, np.zeros(4, f32)
    return True, _plane(orient(n, A), np.asarray(centroid, f64))


def inlier_mask(plane, P, max_dist, M=None, min_normal_cos=0.0):
    """P float32 (m, 3), M float32 (m, 3) or None -> bool (m,): all float32, nothing fused, strict."""
    pl = np.asarray(plane, f32)
    P = np.asarray(P, f32)
    with np.errstate(all="ignore"):
        s = ((pl[0] * P[:, 0] + pl[1] * P[:, 1]) + pl[2] * P[:, 2]) + pl[3]
        assert s.dtype == f32
        m = np.abs(s) < f32(max_dist)
        if M is not None:
            M = np.asarray(M, f32)
            c = (pl[0] * M[:, 0] + pl[1] * M[:, 1]) + pl[2] * M[:, 2]
            m &= np.abs(c) >= f32(min_normal_cos)
    return m


def live_mask(points, normals=None, deleted=None):
    P = np.asarray(points, f32).reshape(-1, 3)
    ok = np.isfinite(P).all(axis=1)
    if deleted is not None:
        ok &= ~np.asarray(deleted, bool)
    if normals is not None:
        M = np.asarray(normals, f32).reshape(-1, 3)
        ok &= np.isfinite(M).all(axis=1) & (M != 0).any(axis=1)
    return ok


def lstsq_frame(points):
    """A group_stats= for the CPU tests: ids -> (centroid, axis 2, eig[0]) by eigh of the covariance (not bit-exact)."""
    P = np.asarray(points, f32).astype(f64).reshape(-1, 3)

    def stats(ids):
        Q = P[ids]
        c = Q.mean(axis=0)
        lam, V = np.linalg.eigh(np.cov((Q - c).T, bias=True))
        return c, V[:, 0], (lam[2] if lam.sum() > 0 else 0.0)
    return stats


def library_frame(tree):
    """A group_stats= from the library's own KDTree.GroupStats."""
    def stats(ids):
        g = tree.GroupStats(ids, [len(ids)])
        return g.centroid[0], g.axes[0, 2], g.eig[0, 0]
    return stats


def segment(points, samples, max_dist, n_hyp, max_planes=1, min_inliers=3, axis=None, min_axis_cos=0.0, normals=None,
            min_normal_cos=0.0, refine=True, deleted=None, hyp_planes=None, group_stats=None):
    P = np.asarray(points, f32).reshape(-1, 3)
    n = len(P)
    M = np.asarray(normals, f32).reshape(-1, 3) if normals is not None else None
    A = Axis(axis, min_axis_cos) if axis is not None else None
    smp = np.asarray(samples, np.uint32).reshape(-1)
    rows = n_hyp * max_planes
    status = np.full(rows, NOT_RUN, np.int32)
    counts = np.zeros(rows, np.int64)
    hyp = np.zeros((rows, 4), f32)
    given = np.asarray(hyp_planes, f32).reshape(rows, 4) if hyp_planes is not None else None
    planes = np.zeros((max_planes, 4), f32)
    sizes = np.zeros(max_planes, np.int64)
    refined = np.zeros(max_planes, np.int32)
    best = np.full(max_planes, -1, np.int64)
    labels = np.full(n, -1, np.int64)
    ids, pre = [], []
    alive = np.flatnonzero(live_mask(P, M, deleted))
    n_planes = 0
    if n_hyp == 0 or n == 0:
        return Result(0, planes, sizes, refined, best, labels, np.zeros(0, np.int64), status.reshape(max_planes, n_hyp),
                      counts.reshape(max_planes, n_hyp), hyp.reshape(max_planes, n_hyp, 4), pre)
    if group_stats is None:
        group_stats = lstsq_frame(P)
    for r in range(max_planes):
        R = len(alive)
        if R < 3:
            break
        Pa, Ma = P[alive], (M[alive] if M is not None else None)
        key = 0
        for h in range(n_hyp):
            row = r * n_hyp + h
            i0, i1, i2 = (sample_index(smp[3 * row + j], R) for j in range(3))
            status[row], hyp[row] = hypothesis(i0, i1, i2, Pa[i0], Pa[i1], Pa[i2], A)
            if status[row] != OK:
                continue
            pl = given[row] if given is not None else hyp[row]
            counts[row] = int(inlier_mask(pl, Pa, max_dist, Ma, min_normal_cos).sum())
            key = max(key, ((int(counts[row]) + 1) << 32) | (~h & 0xffffffff))
        if not key:
            break
        b = ~key & 0xffffffff
        cnt = (key >> 32) - 1
        if cnt < max(int(min_inliers), 3):
            break
        row = r * n_hyp + b
        pl = (given[row] if given is not None else hyp[row]).copy()
        m = inlier_mask(pl, Pa, max_dist, Ma, min_normal_cos)
        pre.append(alive[m].astype(np.int64))
        if refine:
            c, a2, e0 = group_stats(alive[m].astype(np.int64))
            ok, pl2 = refit(c, a2, e0, A)
            if ok:
                m2 = inlier_mask(pl2, Pa, max_dist, Ma, min_normal_cos)
                if int(m2.sum()) >= cnt:
                    pl, m, refined[r] = pl2, m2, 1
        planes[r], best[r], sizes[r] = pl, b, int(m.sum())
        labels[alive[m]] = r
        ids.append(alive[m])
        alive = alive[~m]
        n_planes = r + 1
    ids = np.concatenate(ids).astype(np.int64) if ids else np.zeros(0, np.int64)
    return Result(n_planes, planes, sizes, refined, best, labels, ids, status.reshape(max_planes, n_hyp),
                  counts.reshape(max_planes, n_hyp), hyp.reshape(max_planes, n_hyp, 4), pre)
