"""NumPy restatement of the Normal Distributions Transform extension's contract (include/pcgx.h, "Normal Distributions
Transform").

NO REFERENCE PARITY EXISTS: pcgol has no NDT.  This file is the definition the tests hold the library to.

The map: per occupied voxel v of the bucket grid (grid_addr below restates VoxelGrid.Addr in float32, as bucket_grid.h
has it), in float64 from the float32 inputs widened: o = origin + v resolution, d = p - o, mean_d = sum d / n,
C = (sum d d^T - n mean_d mean_d^T) / (n - 1); invalid when n < max(min_points, 3), all points coincide or trace C <= 0;
valid: C = V diag(l) V^T, l' = max(l, ratio max l), cov = V diag(l') V^T, icov = V diag(1 / l') V^T; mean, cov, icov
rounded to float32 once.

One evaluation: p = Mat4.Transform(T, target) in float32 (synth.transform_points), always applied; the candidates of a
point are its own voxel (1), plus the six face neighbours (7), or the 3 x 3 x 3 block (27), each only if inside the grid
on every axis and valid.  Per pair, in numpy's extended precision rounded to float64 at the end (the contract's float64
up to this file's own error, which that keeps negligible): q = p - mu, m = q^T M q, w = exp(-k2 m / 2),
e = (2 / k2)(1 - w), g_k = w J_k^T M q, H_kl = w J_k^T M J_l.  The 30 sums are {sum e, sum g, sum H upper triangle,
sum w, pairs}.  finish() and gauss_newton_update() are gicp_oracle's (pcgx_math.h restated)."""
import os
import sys

import numpy as np

from pcgol_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gicp_oracle as GO  # noqa: E402
from gicp_oracle import (HKL, P_COUNT, P_G0, P_H0, P_PAIRS, P_VALUE, P_WEIGHT, UPPER, NotEnoughPairs,  # noqa: E402,F401
                         Singular, finish, gauss_newton_update)

f32, f64, ld = np.float32, np.float64, np.longdouble
CHAIN = 9  # ndt_terms.h kNdtChain
IDENTITY = GO._translate(0, 0, 0)


class Grid:
    """The bucket grid's parameters (pcgx_bucket_grid_build's resolution, size, origin)."""

    def __init__(self, resolution, size, origin):
        self.resolution = f32(resolution)
        self.resolution_inv = f32(1) / self.resolution  # voxelgrid.go:21
        self.size = np.asarray(size, np.int64)
        self.origin = np.asarray(origin, f32)

    def addr(self, p):
        """VoxelGrid.Addr (voxelgrid.go:64-79) in float32, vectorised: (ok [n] bool, v [n, 3] int64, addr [n] int64)"""
        p = np.asarray(p, f32).reshape(-1, 3)
        with np.errstate(invalid="ignore", over="ignore"):
            f = ((p - self.origin).astype(f32) * self.resolution_inv).astype(f32) + f32(0.5)
            ok = (f == f) & (f > f32(-9.0e18)) & (f < f32(9.0e18))
            v = np.where(ok, np.trunc(np.where(ok, f, 0)), 0).astype(np.int64)  # Go's float -> int truncation
        ok &= (v >= 0) & (v < self.size)
        ok = ok.all(axis=1)
        a = v[:, 0] + (v[:, 1] + v[:, 2] * self.size[1]) * self.size[0]
        return ok, v, np.where(ok, a, -1)

    def coords(self, addr):
        a = np.asarray(addr, np.int64)
        return np.stack([a % self.size[0], (a // self.size[0]) % self.size[1], a // (self.size[0] * self.size[1])], axis=-1)

    def centre(self, v):
        return self.origin.astype(f64) + np.asarray(v, np.int64).astype(f64) * f64(self.resolution)


def sym6(c6):
    """(n, 6) or (6,) xx, xy, xz, yy, yz, zz -> (n, 3, 3) float64, the input's values as they are"""
    c6 = np.asarray(c6).reshape(-1, 6).astype(f64)
    C = np.empty((len(c6), 3, 3))
    for n, (a, b) in enumerate(UPPER):
        C[:, a, b] = c6[:, n]
        C[:, b, a] = c6[:, n]
    return C


def _six(C):
    return np.array([C[a, b] for a, b in UPPER], f64)


def voxel(points, o, min_points=6, ratio=0.01, parts=1):
    """One voxel's record from its points (float32, bucket order) and its centre o (float64).
    parts > 1: the sums dealt to `parts` accumulators in turn and merged (what a wave does).
    -> dict(count, valid, mean f32 [3], cov6, icov6 float64 [6] (zero when invalid), eig float64 [3] ascending)"""
    p = np.asarray(points, f32).reshape(-1, 3)
    n = len(p)
    d = p.astype(f64) - np.asarray(o, f64)
    s, S = np.zeros(3), np.zeros((3, 3))
    for k in range(parts):
        part = d[k::parts]
        s = s + part.sum(axis=0)
        S = S + part.T @ part
    mean_d = s / n
    out = dict(count=n, valid=0, mean=(np.asarray(o, f64) + mean_d).astype(f32), cov6=np.zeros(6), icov6=np.zeros(6),
               eig=np.zeros(3))
    if n < max(int(min_points), 3) or np.all(p == p[0]):
        return out
    C = (S - n * np.outer(mean_d, mean_d)) / (n - 1)
    if not np.trace(C) > 0.0:
        return out
    l, V = np.linalg.eigh(C)
    lc = np.maximum(l, f64(f32(ratio)) * l.max())
    out.update(valid=1, cov6=_six((V * lc) @ V.T), icov6=_six((V / lc) @ V.T), eig=l)
    return out


def build_map(grid, points, min_points=6, ratio=0.01, parts=1):
    """-> dict(grid, addr int64 [m] ascending, count, valid int32 [m], mean f32 [m, 3], cov6, icov6 f32 [m, 6], and the
    float64 cov6_64 / icov6_64 before the rounding)"""
    pts = np.asarray(points, f32).reshape(-1, 3)
    ok, _, a = grid.addr(pts)
    ids = np.nonzero(ok)[0]
    order = ids[np.argsort(a[ids], kind="stable")]  # a voxel's points in insertion order
    addrs, starts = np.unique(a[order], return_index=True)
    ends = list(starts[1:]) + [len(order)]
    recs = [voxel(pts[order[s:e]], grid.centre(grid.coords(ad)), min_points, ratio, parts)
            for ad, s, e in zip(addrs, starts, ends)]
    m = len(recs)
    c64 = np.array([r["cov6"] for r in recs], f64).reshape(m, 6)
    i64 = np.array([r["icov6"] for r in recs], f64).reshape(m, 6)
    return dict(grid=grid, addr=addrs.astype(np.int64), count=np.array([r["count"] for r in recs], np.int32),
                valid=np.array([r["valid"] for r in recs], np.int32),
                mean=np.array([r["mean"] for r in recs], f32).reshape(m, 3), cov6=c64.astype(f32), icov6=i64.astype(f32),
                cov6_64=c64, icov6_64=i64)


def k2_of(outlier_ratio, resolution):
    """Magnusson's constants -> k2 (float64, from extended precision); None: not usable (PCGX_E_INVALID)"""
    o, res = ld(f32(outlier_ratio)), ld(f32(resolution))
    if not (o > 0 and o < 1):
        return None
    with np.errstate(all="ignore"):
        c1 = ld(10) * (ld(1) - o)
        c2 = o / (res * res * res)
        d3 = -np.log(c2)
        d1 = -np.log(c1 + c2) - d3
        k2 = f64(ld(-2) * np.log((-np.log(c1 * np.exp(ld(-0.5)) + c2) - d3) / d1))
    return float(k2) if np.isfinite(k2) and k2 > 0 else None


def offsets(neighbors):
    if neighbors == 1:
        return [(0, 0, 0)]
    if neighbors == 7:
        return [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    if neighbors == 27:
        return [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    raise ValueError("neighbors must be 1, 7 or 27")


def pairs(map_, p, neighbors):
    """(point index, valid-voxel index into map_'s arrays) of every pair of the moved points p (float32)"""
    g = map_["grid"]
    ok, v, _ = g.addr(p)
    vi = np.nonzero(map_["valid"] != 0)[0]
    vaddr = map_["addr"][vi]
    pi_all, vj_all = [], []
    idx = np.nonzero(ok)[0]
    for off in offsets(neighbors):
        vv = v[idx] + np.asarray(off, np.int64)
        inside = np.all((vv >= 0) & (vv < g.size), axis=1)  # (a neighbour beyond the grid is nobody's voxel)
        a = vv[:, 0] + (vv[:, 1] + vv[:, 2] * g.size[1]) * g.size[0]
        pos = np.searchsorted(vaddr, a)
        hit = inside & (pos < len(vaddr))
        hit[hit] &= vaddr[pos[hit]] == a[hit]
        pi_all.append(idx[hit])
        vj_all.append(vi[pos[hit]])
    return np.concatenate(pi_all), np.concatenate(vj_all)


def pair_terms(p, mean, icov6, k2):
    """p, mean (m, 3) float32; icov6 (m, 6) float32 -> (terms (m, 30), absterms (m, 30)): absterms with the weight's
    share taken as w (1 + k2 m / 2)"""
    p = np.asarray(p, f32).astype(ld)
    q = p - np.asarray(mean, f32).astype(ld)
    M = sym6(icov6).astype(ld)
    n = len(p)
    k2 = ld(k2)
    terms, absterms = np.zeros((n, P_COUNT)), np.zeros((n, P_COUNT))
    if n == 0:
        return terms, absterms
    J = GO.jacobians(p)
    Mq = np.einsum("nab,nb->na", M, q)
    aMq = np.einsum("nab,nb->na", np.abs(M), np.abs(q))
    mm = np.einsum("na,na->n", q, Mq)
    a = k2 * mm / ld(2)
    w = np.exp(-a)
    wa = w * (ld(1) + np.abs(a))
    terms[:, P_VALUE] = (ld(2) / k2) * (ld(1) - w)
    absterms[:, P_VALUE] = (ld(2) / k2) * (np.abs(ld(1) - w) + wa)
    terms[:, P_G0:P_G0 + 6] = w[:, None] * np.einsum("nka,na->nk", J, Mq)
    absterms[:, P_G0:P_G0 + 6] = wa[:, None] * np.einsum("nka,na->nk", np.abs(J), aMq)
    JM = np.einsum("nka,nab->nkb", J, M)
    aJM = np.einsum("nka,nab->nkb", np.abs(J), np.abs(M))
    for i, (k, l) in enumerate(HKL):
        terms[:, P_H0 + i] = w * np.einsum("nb,nb->n", JM[:, k], J[:, l])
        absterms[:, P_H0 + i] = wa * np.einsum("nb,nb->n", aJM[:, k], np.abs(J[:, l]))
    terms[:, P_WEIGHT] = w
    absterms[:, P_WEIGHT] = wa
    terms[:, P_PAIRS] = 1.0
    absterms[:, P_PAIRS] = 1.0
    return terms, absterms


def sums(map_, target, trans=None, neighbors=7, outlier_ratio=0.55):
    """One evaluation at pose trans (None: the identity, applied all the same).
    -> dict(sums (30,), A (30,), pairs, k2)"""
    k2 = k2_of(outlier_ratio, map_["grid"].resolution)
    if k2 is None:
        raise ValueError("no usable k2")
    target = np.ascontiguousarray(target, f32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):  # (an infinite coordinate times the matrix's zeros is NaN: off-grid)
        p = synth.transform_points(IDENTITY if trans is None else np.asarray(trans, f32).reshape(16), target)
    pi, vj = pairs(map_, p, neighbors)
    t, a = pair_terms(p[pi], map_["mean"][vj], map_["icov6"][vj], k2)
    return dict(sums=t.sum(axis=0), A=a.sum(axis=0), pairs=len(pi), k2=k2)


def fit(map_, target, neighbors=7, outlier_ratio=0.55, min_pairs=0, threshold=None, damping=0.0, max_iter=0, init=None,
        trace=None):
    """The Fit loop: evaluate, finish (the plane tail), gauss_newton_update.
    -> dict(trans, num_iteration, evaluated); trace: a list that receives (trans before the evaluation, sums dict)"""
    trans = IDENTITY.copy() if init is None else np.asarray(init, f32).reshape(16).copy()
    it, num, ev = 0, 0, None
    for _ in range(max_iter or 20):
        num += 1
        s = sums(map_, target, trans, neighbors, outlier_ratio)
        if trace is not None:
            trace.append((trans.copy(), s))
        ev = finish(s["sums"], min_pairs)
        trans, conv, it = gauss_newton_update(trans, it, ev, threshold, damping, max_iter)
        if conv:
            break
    return dict(trans=trans, num_iteration=num, evaluated=ev)


# ---- the prototype scene (tests/test_ndt_oracle.py pins its figures; the GPU tests run the library on it)
TRUTH_ROT = (0.03, -0.021, 0.039)
TRUTH_T = (0.1, -0.06, 0.04)


def truth_pose():
    """Translate(t) * Rodrigues(w) in the library's float32 arithmetic"""
    return GO._mat4_mul(GO._translate(*TRUTH_T), GO._rodrigues(np.asarray(TRUTH_ROT, f32)))


def inverse_pose(m):
    return np.ascontiguousarray(np.linalg.inv(np.asarray(m, f64).reshape(4, 4).T).T.reshape(-1).astype(f32))


def prototype_scene():
    """base: surface_cloud(6000, 4, 21); target: surface_cloud(3000, 4, 22) moved by the inverse of the truth pose, so
    that the Fit's answer is the truth pose; grid: origin (-1, -1, -2), resolution 0.5, size (13, 13, 9)."""
    base = synth.surface_cloud(6000, 4.0, 21)[0]
    truth = truth_pose()
    target = synth.transform_points(inverse_pose(truth), synth.surface_cloud(3000, 4.0, 22)[0])
    return dict(base=base, target=target, truth=truth, grid=Grid(0.5, (13, 13, 9), (-1.0, -1.0, -2.0)))


def translation_error(trans, truth):
    return float(np.linalg.norm(np.asarray(trans, f64)[12:15] - np.asarray(truth, f64)[12:15]))
