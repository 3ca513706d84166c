"""The contract of pcgx_kdtree_shapes (include/pcgx.h, "shapes") restated in NumPy: the live points, the rounds, the
partner rule over Range's set, the hypothesis of two oriented points (float64, one rounding an operation), the strict
float32 inlier test without a square root, the first best, the one refit and the outputs.  `segment` takes `hyp_shapes=`
so that counts can be checked at the library's own record bits, and `lib_shapes=` / `lib_refined=`: where the library
kept a refitted record, the recount and the decision are made at the library's bits, and `refits` holds the oracle's own
refit (exact sums by math.fsum, a float64 solve) with the tolerance a refitted number may differ by.  `range_of=`
(seed id -> ids) replaces the brute-force ball as Range's set: on a handle that holds non-finite points Range is the
reference's walk of a tree with NaN keys in it, which is not the ball, and the contract names Range's set."""
import collections
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_oracle as PO  # noqa: E402

f32, f64, u32 = np.float32, np.float64, np.uint32
SPHERE, CYLINDER = 0, 1
NOT_RUN, OK, NO_PARTNER, DEGENERATE, AXIS, RADIUS = -1, 0, 1, 2, 3, 4
PARALLEL_EPS = 1e-12
PIVOT_EPS = 1e-12

Result = collections.namedtuple("Result", "n_shapes shapes sizes refined best labels ids status counts hyp_shapes "
                                          "pre_ids partners refits")
# pre_ids: per found round, the best hypothesis's inliers; partners: (max_shapes, n_hyp) the partner's id or -1;
# refits: per found round None or Refit
Refit = collections.namedtuple("Refit", "ok rec kappa n tol")

Axis, sample_index, live_mask = PO.Axis, PO.sample_index, PO.live_mask


def mix(u1, ids):
    """the partner rule's x of the word u1 and the ids (uint32 arithmetic) -> uint32 array"""
    with np.errstate(over="ignore"):
        x = u32(u1) ^ (np.asarray(ids).astype(u32) * u32(0x9E3779B1))
        x ^= x >> u32(16)
        x *= u32(0x85EBCA6B)
        x ^= x >> u32(13)
        x *= u32(0xC2B2AE35)
        x ^= x >> u32(16)
    return x


def partner(u1, candidates):
    """the candidate with the smallest (x, id); -1 where there is none"""
    c = np.asarray(candidates, np.int64).reshape(-1)
    if len(c) == 0:
        return -1
    key = (mix(u1, c).astype(np.uint64) << np.uint64(32)) | c.astype(np.uint64)
    return int(c[np.argmin(key)])


def range_set(P, q, radius):
    """Range's set: the float32 DistSq (dx dx + dy dy) + dz dz, d = p - q, strictly below the float32 radius * radius"""
    P = np.asarray(P, f32)
    q = np.asarray(q, f32)
    with np.errstate(all="ignore"):
        d = P - q
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return d2 < f32(radius) * f32(radius)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _pos(v):
    return v if v > 0.0 else f64(0.0)


def _store(v):
    rec = np.asarray(v, f64).astype(f32)
    if not np.isfinite(rec).all():
        return False, np.zeros(8, f32)
    return True, rec


def _rho(p, q, a):
    v = p - q
    t = _dot(v, a)
    return np.sqrt(_pos(_dot(v, v) - t * t))


def _canonical(c, a):
    return c - _dot(c, a) * a


def hypothesis(kind, has_partner, p0, n0, p1, n1, A=None, r_min=0.0, r_max=np.inf):
    """-> (status, record float32 (8,)): the shape of two oriented points"""
    zero = np.zeros(8, f32)
    if not has_partner:
        return NO_PARTNER, zero
    with np.errstate(all="ignore"):
        p0, n0, p1, n1 = (np.asarray(v, f32).astype(f64) for v in (p0, n0, p1, n1))
        w = p0 - p1
        a_, b_, c_, d_, e_ = _dot(n0, n0), _dot(n0, n1), _dot(n1, n1), _dot(n0, w), _dot(n1, w)
        den = a_ * c_ - b_ * b_
        if not den > PARALLEL_EPS * (a_ * c_):
            return DEGENERATE, zero
        s, t = (b_ * e_ - c_ * d_) / den, (a_ * e_ - b_ * d_) / den
        m = 0.5 * ((p0 + s * n0) + (p1 + t * n1))
        v = np.zeros(8, f64)
        if kind == SPHERE:
            u0, u1 = p0 - m, p1 - m
            r = 0.5 * (np.sqrt(_dot(u0, u0)) + np.sqrt(_dot(u1, u1)))
            v[:3] = m
        else:
            c = np.array([n0[1] * n1[2] - n0[2] * n1[1], n0[2] * n1[0] - n0[0] * n1[2], n0[0] * n1[1] - n0[1] * n1[0]])
            a = c / np.sqrt(_dot(c, c))
            if not PO.axis_ok(a, A):
                return AXIS, zero
            a = PO.orient(a, A)
            q = _canonical(m, a)
            r = 0.5 * (_rho(p0, q, a) + _rho(p1, q, a))
            v[:3], v[4:7] = q, a
        v[3] = r
        if not (r >= f64(f32(r_min)) and r <= f64(f32(r_max))):
            return RADIUS, zero
        ok, rec = _store(v)
        return (OK, rec) if ok else (RADIUS, zero)


def band(r, max_dist):
    """-> (lo2, hi2) float32"""
    with np.errstate(all="ignore"):
        r, md = f32(r), f32(max_dist)
        lo, hi = f32(r - md), f32(r + md)
        return (f32(lo * lo) if lo > 0 else f32(-1.0)), f32(hi * hi)


def inlier_mask(kind, rec, P, max_dist, M, min_normal_cos=0.0):
    """P, M float32 (m, 3) -> bool (m,): all float32, nothing fused, no square root, strict"""
    rec = np.asarray(rec, f32)
    P, M = np.asarray(P, f32), np.asarray(M, f32)
    lo2, hi2 = band(rec[3], max_dist)
    with np.errstate(all="ignore"):
        vx, vy, vz = P[:, 0] - rec[0], P[:, 1] - rec[1], P[:, 2] - rec[2]
        d2 = (vx * vx + vy * vy) + vz * vz
        if kind == CYLINDER:
            t = (vx * rec[4] + vy * rec[5]) + vz * rec[6]
            d2 = d2 - t * t
        assert d2.dtype == f32
        m = (d2 < hi2) & (d2 > lo2)
        if f32(min_normal_cos) != 0:
            c2 = f32(min_normal_cos) * f32(min_normal_cos)
            g = (M[:, 0] * vx + M[:, 1] * vy) + M[:, 2] * vz
            if kind == CYLINDER:
                g = g - t * ((M[:, 0] * rec[4] + M[:, 1] * rec[5]) + M[:, 2] * rec[6])
            assert g.dtype == f32
            m &= g * g >= c2 * d2
    return m


def cylinder_frame(a):
    a = np.asarray(a, f64)
    m = np.abs(a)
    k = 0 if (m[0] <= m[1] and m[0] <= m[2]) else (1 if m[1] <= m[2] else 2)
    c = np.zeros(3, f64)
    c[k] = 1.0
    x = np.array([a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]])
    e1 = x / np.sqrt(_dot(x, x))
    e2 = np.array([a[1] * e1[2] - a[2] * e1[1], a[2] * e1[0] - a[0] * e1[2], a[0] * e1[1] - a[1] * e1[0]])
    return e1, e2


def refit_coords(kind, rec, pts):
    """the coordinates the sums run over, float64 (m, 3): p - pivot, or its two components across the axis and a 0"""
    rec = np.asarray(rec, f32).astype(f64)
    v = np.asarray(pts, f32).astype(f64).reshape(-1, 3) - rec[:3]
    if kind == SPHERE:
        return v
    e1, e2 = cylinder_frame(rec[4:7])
    x = np.zeros_like(v)
    x[:, 0] = (v[:, 0] * e1[0] + v[:, 1] * e1[1]) + v[:, 2] * e1[2]
    x[:, 1] = (v[:, 0] * e2[0] + v[:, 1] * e2[1]) + v[:, 2] * e2[2]
    return x


def refit_sums(x):
    """the 13 sums, each added exactly (math.fsum) over the terms rounded as the contract rounds them"""
    q = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
    cols = [x[:, 0], x[:, 1], x[:, 2], x[:, 0] * x[:, 0], x[:, 0] * x[:, 1], x[:, 0] * x[:, 2], x[:, 1] * x[:, 1],
            x[:, 1] * x[:, 2], x[:, 2] * x[:, 2], q * x[:, 0], q * x[:, 1], q * x[:, 2], q]
    return np.array([math.fsum(c.tolist()) for c in cols], f64)


def normal_system(kind, n, s):
    d = 3 if kind == SPHERE else 2
    at = [[3, 4, 5], [4, 6, 7], [5, 7, 8]]
    M, b = np.zeros((d + 1, d + 1), f64), np.zeros(d + 1, f64)
    for i in range(d):
        for j in range(d):
            M[i, j] = 4.0 * s[at[i][j]]
        M[i, d] = M[d, i] = 2.0 * s[i]
        b[i] = 2.0 * s[9 + i]
    M[d, d], b[d] = f64(n), s[12]
    return M, b


def refit_from_sums(kind, rec, n, s, r_min=0.0, r_max=np.inf):
    """-> (ok, record): the contract's solve of the sums s over n points about the record rec"""
    zero = np.zeros(8, f32)
    rec = np.asarray(rec, f32)
    with np.errstate(all="ignore"):
        M, b = normal_system(kind, n, np.asarray(s, f64))
        m = len(b)
        d = m - 1
        big = max(0.0, max(M[i, i] for i in range(m)))
        L, y = np.zeros((m, m), f64), np.zeros(m, f64)
        for j in range(m):
            piv = M[j, j]
            for k in range(j):
                piv = piv - L[j, k] * L[j, k]
            if not piv > PIVOT_EPS * big:
                return False, zero
            L[j, j] = np.sqrt(piv)
            for i in range(j + 1, m):
                v = M[i, j]
                for k in range(j):
                    v = v - L[i, k] * L[j, k]
                L[i, j] = v / L[j, j]
        for i in range(m):
            v = b[i]
            for k in range(i):
                v = v - L[i, k] * y[k]
            y[i] = v / L[i, i]
        for i in range(m - 1, -1, -1):
            v = y[i]
            for k in range(i + 1, m):
                v = v - L[k, i] * y[k]
            y[i] = v / L[i, i]
        u = np.array([y[0], y[1], y[2] if d == 3 else 0.0])
        r2 = y[d] + _dot(u, u)
        if not r2 > 0.0:
            return False, zero
        r = np.sqrt(r2)
        if not (r >= f64(f32(r_min)) and r <= f64(f32(r_max))):
            return False, zero
        v = np.zeros(8, f64)
        v[3] = r
        piv = rec[:3].astype(f64)
        if kind == SPHERE:
            v[:3] = piv + u
        else:
            a = rec[4:7].astype(f64)
            e1, e2 = cylinder_frame(a)
            c = (piv + u[0] * e1) + u[1] * e2
            v[:3], v[4:7] = _canonical(c, a), a
        return _store(v)


def refit(kind, rec, pts, r_min=0.0, r_max=np.inf):
    """-> Refit(ok, record, kappa, n, tol): the refit over the points pts (the inliers in ascending id), the condition
    number of the column-scaled normal matrix, and what a refitted number of a float64 implementation that adds in
    another order may differ by: max(one float32 ulp at the record's scale, n kappa 2^-52 times that scale)"""
    x = refit_coords(kind, rec, pts)
    n = len(x)
    s = refit_sums(x)
    ok, out = refit_from_sums(kind, rec, n, s, r_min, r_max)
    M, _ = normal_system(kind, n, s)
    with np.errstate(all="ignore"):
        dg = np.sqrt(np.abs(np.diag(M)))
        kappa = float(np.linalg.cond(M / np.outer(dg, dg))) if np.all(dg > 0) else np.inf
    scale = float(np.abs(out[:4]).max()) if ok else 0.0
    ulp = float(np.spacing(f32(scale))) if ok else 0.0
    return Refit(ok, out, kappa, n, max(ulp, n * kappa * 2.0 ** -52 * scale))


def segment(points, normals, kind, samples, max_dist, n_hyp, max_shapes=1, min_inliers=2, sample_radius=0.0, r_min=0.0,
            r_max=np.inf, axis=None, min_axis_cos=0.0, min_normal_cos=0.0, refine=True, deleted=None, hyp_shapes=None,
            lib_shapes=None, lib_refined=None, range_of=None):
    P = np.asarray(points, f32).reshape(-1, 3)
    M = np.asarray(normals, f32).reshape(-1, 3)
    n = len(P)
    A = Axis(axis, min_axis_cos) if axis is not None else None
    smp = np.asarray(samples, u32).reshape(-1)
    rows = n_hyp * max_shapes
    status = np.full(rows, NOT_RUN, np.int32)
    counts = np.zeros(rows, np.int64)
    hyp = np.zeros((rows, 8), f32)
    partners = np.full(rows, -1, np.int64)
    given = np.asarray(hyp_shapes, f32).reshape(rows, 8) if hyp_shapes is not None else None
    shapes = np.zeros((max_shapes, 8), f32)
    sizes = np.zeros(max_shapes, np.int64)
    refined = np.zeros(max_shapes, np.int32)
    best = np.full(max_shapes, -1, np.int64)
    labels = np.full(n, -1, np.int64)
    ids, pre, refits = [], [], []
    left = live_mask(P, M, deleted)
    n_shapes = 0

    def done():
        out = np.concatenate(ids).astype(np.int64) if ids else np.zeros(0, np.int64)
        return Result(n_shapes, shapes, sizes, refined, best, labels, out, status.reshape(max_shapes, n_hyp),
                      counts.reshape(max_shapes, n_hyp), hyp.reshape(max_shapes, n_hyp, 8), pre,
                      partners.reshape(max_shapes, n_hyp), refits)
    if n_hyp == 0 or n == 0:
        return done()
    gone = np.asarray(deleted, bool) if deleted is not None else np.zeros(n, bool)
    for r in range(max_shapes):
        alive = np.flatnonzero(left)
        R = len(alive)
        if R < 2:
            break
        Pa, Ma = P[alive], M[alive]
        key = 0
        for h in range(n_hyp):
            row = r * n_hyp + h
            i0 = int(alive[sample_index(smp[2 * row], R)])
            if f32(sample_radius) > 0:
                if range_of is None:
                    inside = range_set(P, P[i0], sample_radius)
                else:
                    inside = np.zeros(n, bool)
                    inside[np.asarray(range_of(i0), np.int64)] = True
                cand = left & ~gone & inside
                cand[i0] = False
                i1 = partner(smp[2 * row + 1], np.flatnonzero(cand))
            else:
                i1 = int(alive[sample_index(smp[2 * row + 1], R)])
            has = i1 >= 0 and i1 != i0
            partners[row] = i1 if has else -1
            j1 = i1 if has else i0
            status[row], hyp[row] = hypothesis(kind, has, P[i0], M[i0], P[j1], M[j1], A, r_min, r_max)
            if status[row] != OK:
                continue
            rec = given[row] if given is not None else hyp[row]
            counts[row] = int(inlier_mask(kind, rec, Pa, max_dist, Ma, min_normal_cos).sum())
            key = max(key, ((int(counts[row]) + 1) << 32) | (~h & 0xffffffff))
        if not key:
            break
        b = ~key & 0xffffffff
        cnt = (key >> 32) - 1
        if cnt < max(int(min_inliers), 2):
            break
        row = r * n_hyp + b
        rec = (given[row] if given is not None else hyp[row]).copy()
        m = inlier_mask(kind, rec, Pa, max_dist, Ma, min_normal_cos)
        pre.append(alive[m].astype(np.int64))
        refits.append(None)
        if refine:
            f = refits[-1] = refit(kind, rec, P[alive[m]], r_min, r_max)
            if f.ok:
                # where the library kept a refitted record, the recount is made at its bits (the test compares them
                # with f.rec inside f.tol)
                rec2 = np.asarray(lib_shapes, f32)[r] if lib_shapes is not None and lib_refined[r] else f.rec
                m2 = inlier_mask(kind, rec2, Pa, max_dist, Ma, min_normal_cos)
                if int(m2.sum()) >= cnt:
                    rec, m, refined[r] = rec2.copy(), m2, 1
        shapes[r], best[r], sizes[r] = rec, b, int(m.sum())
        labels[alive[m]] = r
        ids.append(alive[m])
        left[alive[m]] = False
        n_shapes = r + 1
    return done()
