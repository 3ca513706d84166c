"""NumPy restatement of boundary detection (include/pcgx.h, "boundary points"; csrc/boundary.hip,
csrc/boundary_terms.h).

No reference counterpart exists: this is the contract itself, in float64 over brute-force lists.
  N(i)      = the points p of the cloud (deleted ones left out) with DistSq(p, point i) < r*r, DistSq the reference's
              float32 (dx*dx + dy*dy) + dz*dz; count = |N(i)|;
  evaluated = i in N(i), and the normal's components finite and not all zero, and count >= max(min_neighbors, 1);
  frame     = float64 from the float32 normal n: e the unit vector of the axis where |n| is smallest (a tie: the lowest
              axis), u = n x e, v = n x u, every component a difference of two products; not normalised;
  direction = d = p - q in float64, a = (d.x u.x + d.y u.y) + d.z u.z, b likewise with v; a == b == 0: no sector;
  sector    = 16 Q + #{k in 1..15 : y >= x T[k]} after the quarter turn Q that brings (a, b) to x > 0, y >= 0, T[k] the
              float64 nearest tan(k pi / 32);
  mask      = OR of 1 << sector over N(i); gap = the longest cyclic run of zero bits (64 for mask 0);
  boundary  = evaluated and gap >= min_gap.
A point that is not evaluated has mask 0 and gap -1; its count is |N(i)| when it met itself and its normal is usable
(only min_neighbors failed), else 0: nothing is enumerated for a normal that gives no frame."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_oracle as NO  # noqa: E402

f32, f64, u64 = np.float32, np.float64, np.uint64

SECTORS = 64
# T[k], k = 1..15: the float64 nearest tan(k pi / 32) (T[0] is a placeholder); the terms header has the same 15 numbers
T = np.array([0.0, 0.09849140335716425, 0.198912367379658, 0.3033466836073424, 0.41421356237309503, 0.5345111359507917,
              0.6681786379192989, 0.8206787908286604, 1.0, 1.2185035255879764, 1.496605762665489, 1.8708684117893895,
              2.414213562373095, 3.2965582089383205, 5.027339492125848, 10.15317038760886], f64)


def usable(normals):
    n = np.asarray(normals, f32).reshape(-1, 3)
    return np.isfinite(n).all(axis=1) & (n != 0).any(axis=1)


def frame(normals):
    """-> (u, v) float64 (m, 3); rows of unusable normals hold whatever the arithmetic gives"""
    n = np.asarray(normals, f32).reshape(-1, 3).astype(f64)
    with np.errstate(invalid="ignore", over="ignore"):
        axis = np.argmin(np.abs(np.where(np.isnan(n), np.inf, n)), axis=1)  # the first smallest: the lowest axis
        e = np.zeros_like(n)
        e[np.arange(len(n)), axis] = 1.0

        def cross(p, q):
            return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2],
                             p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], axis=1)
        u = cross(n, e)
        v = cross(n, u)
    return u, v


def direction(u, v, p, q):
    """a, b of neighbours p (m, 3) float32 seen from q (m, 3) float32 in the frames u, v (m, 3)"""
    d = np.asarray(p, f32).astype(f64) - np.asarray(q, f32).astype(f64)
    a = (d[:, 0] * u[:, 0] + d[:, 1] * u[:, 1]) + d[:, 2] * u[:, 2]
    b = (d[:, 0] * v[:, 0] + d[:, 1] * v[:, 1]) + d[:, 2] * v[:, 2]
    return a, b


def sector(a, b):
    """-> int64: 0..63, or -1 where a == b == 0"""
    a, b = np.asarray(a, f64).reshape(-1), np.asarray(b, f64).reshape(-1)
    q0 = (a > 0) & (b >= 0)
    q1 = (a <= 0) & (b > 0)
    q2 = (a < 0) & (b <= 0)
    q3 = (a >= 0) & (b < 0)
    none = (a == 0) & (b == 0)
    assert np.all(q0.astype(int) + q1 + q2 + q3 + none == 1)
    Q = np.select([q0, q1, q2, q3], [0, 1, 2, 3], -1)
    x = np.select([q0, q1, q2, q3], [a, b, -a, -b], 1.0)
    y = np.select([q0, q1, q2, q3], [b, -a, -b, a], 0.0)
    s = np.zeros(len(a), np.int64)
    with np.errstate(over="ignore"):  # (a and b of a neighbourhood's members cannot overflow; a test's own inputs may)
        for k in range(1, 16):
            s += y >= x * T[k]
    return np.where(none, -1, 16 * Q + s)


def gap(masks):
    """the longest cyclic run of zero bits of every uint64 mask -> int64 (0..64)"""
    m = np.asarray(masks, u64).reshape(-1)
    z = ((m[:, None] >> np.arange(64, dtype=u64)[None, :]) & u64(1)) == 0
    zz = np.concatenate([z, z], axis=1)
    run = np.zeros(len(m), np.int64)
    best = np.zeros(len(m), np.int64)
    for j in range(128):
        run = (run + 1) * zz[:, j]
        best = np.maximum(best, run)
    return np.minimum(best, 64)


def pair_sectors(points, normals, offs, ids, sel=None, chunk=1 << 21):
    """the sector (int8, -1: none) of every pair of CSR lists: list k is N(sel[k]) (sel: default every id)"""
    P = np.asarray(points, f32).reshape(-1, 3)
    u, v = frame(normals)
    sel = np.arange(len(P)) if sel is None else np.asarray(sel, np.int64)
    offs, ids = np.asarray(offs, np.int64), np.asarray(ids, np.int64)
    qi = sel[np.repeat(np.arange(len(sel)), np.diff(offs))]
    out = np.full(len(ids), -1, np.int8)
    todo = np.nonzero(usable(normals)[qi])[0]  # (a point without a frame is not evaluated: its pairs have no sector)
    for s in range(0, len(todo), chunk):
        k = todo[s:s + chunk]
        q, j = qi[k], ids[k]
        a, b = direction(u[q], v[q], P[j], P[q])
        out[k] = sector(a, b)
    return out


def from_sectors(normals, offs, ids, sectors, min_gap=16, min_neighbors=1, sel=None, deleted=None):
    """the rule over CSR lists and their pairs' sectors -> dict(ids, gaps, masks, counts, evaluated).  Ids outside `sel`
    must have unusable normals (nothing is evaluated there); `deleted` ids leave every list, their own included."""
    nrm = np.asarray(normals, f32).reshape(-1, 3)
    n = len(nrm)
    ok = usable(nrm)
    sel = np.arange(n) if sel is None else np.asarray(sel, np.int64)
    assert not ok[np.setdiff1d(np.arange(n), sel)].any()
    offs, ids = np.asarray(offs, np.int64), np.asarray(ids, np.int64)
    qi = sel[np.repeat(np.arange(len(sel)), np.diff(offs))]
    keep = ok[qi]
    if deleted is not None and len(deleted):
        gone = np.zeros(n, bool)
        gone[np.asarray(deleted, np.int64)] = True
        keep &= ~gone[ids] & ~gone[qi]
    qi, ids, sectors = qi[keep], ids[keep], np.asarray(sectors)[keep].astype(np.int64)
    met = np.bincount(qi[ids == qi], minlength=n) > 0
    counts = np.where(met, np.bincount(qi, minlength=n), 0).astype(np.int32)
    hit = np.zeros(n * SECTORS, bool)
    has = sectors >= 0
    hit[qi[has] * SECTORS + sectors[has]] = True
    masks = (hit.reshape(n, SECTORS).astype(u64) << np.arange(SECTORS, dtype=u64)[None, :]).sum(axis=1, dtype=u64)
    evaluated = met & ok & (counts >= max(int(min_neighbors), 1))
    masks = np.where(evaluated, masks, u64(0))
    gaps = np.where(evaluated, gap(masks), -1).astype(np.int32)
    out = np.nonzero(evaluated & (gaps >= int(min_gap)))[0].astype(np.int64)
    return dict(ids=out, gaps=gaps, masks=masks, counts=counts, evaluated=evaluated)


def from_lists(points, normals, offs, ids, min_gap=16, min_neighbors=1, sel=None, deleted=None):
    return from_sectors(normals, offs, ids, pair_sectors(points, normals, offs, ids, sel), min_gap, min_neighbors, sel,
                        deleted)


def boundary(points, normals, radius, min_gap=16, min_neighbors=1, deleted=None):
    """brute force end to end; a deleted point becomes NaN (never DistSq < bound: nobody's neighbour, not its own)"""
    p = np.array(points, f32).reshape(-1, 3)
    if deleted is not None and len(deleted):
        p[np.asarray(deleted, np.int64)] = np.nan
    with np.errstate(invalid="ignore"):
        offs, ids = NO.brute_force_lists(p, p, radius)
    return from_lists(p, normals, offs, ids, min_gap, min_neighbors)


def check(ref, ids, gaps, masks, counts, what=""):
    """the library's four outputs against an oracle result, exactly"""
    assert np.array_equal(np.asarray(counts, np.int64), ref["counts"].astype(np.int64)), (what, "counts")
    bad = np.nonzero(np.asarray(masks, u64) != ref["masks"])[0]
    assert len(bad) == 0, (what, "masks", bad[:10], [hex(int(x)) for x in np.asarray(masks, u64)[bad[:3]]],
                           [hex(int(x)) for x in ref["masks"][bad[:3]]])
    assert np.array_equal(np.asarray(gaps, np.int64), ref["gaps"].astype(np.int64)), (what, "gaps")
    assert np.array_equal(np.asarray(ids, np.int64), ref["ids"]), (what, "ids")
