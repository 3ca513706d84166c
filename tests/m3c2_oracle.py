"""The contract of the cylinder statistics and of M3C2's finish (include/pcgx.h, "cylinder statistics" and "M3C2")
restated in NumPy float64, brute force over all (cylinder, point) pairs.  float64 from the float32 inputs widened, the
operation order as written there, every product and sum rounded once (NumPy fuses nothing), no square root and no
division in the member test and the terms; the sums are the exact sums of the rounded terms (math.fsum), and `mag` is
what the summation bound n 2^-53 sum|term| is made of.  The finish divides and takes roots, IEEE on both sides."""
import math

import numpy as np

import rays_oracle as RO

f32, f64 = np.float32, np.float64
CHUNK = 32  # cylinders per block of the brute force


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, f32)
    return a if shape is None else a.reshape(shape)


def cyl_terms(o, d, rho, half_length):
    """dd, rr dd, ll dd, usable -- per cylinder."""
    o, d = _f32(o, (-1, 3)).astype(f64), _f32(d, (-1, 3)).astype(f64)
    with np.errstate(all="ignore"):
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        rr = f64(f32(rho)) * f64(f32(rho))
        ll = f64(f32(half_length)) * f64(f32(half_length))
        usable = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (dd != 0.0)
    return dd, rr * dd, ll * dd, usable


def members(points, o, d, rho, half_length, deleted=None):
    """(member (m, n) bool, a (m, n) float64): a and cc are rays_oracle.pair_terms' -- the ray queries' expressions."""
    points = _f32(points, (-1, 3))
    dd, rrdd, lldd, usable = cyl_terms(o, d, rho, half_length)
    a, cc = RO.pair_terms(o, d, points)
    live = np.isfinite(points).all(1)
    if deleted is not None and len(deleted):
        live = live.copy()
        live[np.asarray(deleted, np.int64)] = False
    with np.errstate(all="ignore"):
        m = (cc <= rrdd[:, None]) & (a * a <= lldd[:, None])
    return m & usable[:, None] & live[None, :], a


def stats(points, o, d, rho, half_length, deleted=None):
    """-> (counts int32 (m,), sums float64 (m, 2): the exact sums, rounded once, terms: per cylinder its members' a in
    id order)."""
    o, d = _f32(o, (-1, 3)), _f32(d, (-1, 3))
    m = len(o)
    counts, sums, terms = np.zeros(m, np.int32), np.zeros((m, 2), f64), [np.zeros(0, f64)] * m
    if len(_f32(points, (-1, 3))) == 0:
        return counts, sums, terms
    for f in range(0, m, CHUNK):
        e = min(f + CHUNK, m)
        mem, a = members(points, o[f:e], d[f:e], rho, half_length, deleted)
        counts[f:e] = mem.sum(1)
        for i in range(f, e):
            t = a[i - f][mem[i - f]]
            terms[i] = t
            if len(t):
                sums[i] = math.fsum(t), math.fsum(t * t)
    return counts, sums, terms


def sums_within_bound(got, terms):
    """Is every got[i] = (S1, S2) within n 2^-53 sum|term| of the EXACT sum of cylinder i's terms (the bound of any
    summation order while n n < 2^53)?  The deviation is exact too: fsum over the terms and -got.  -> the indices that
    are not."""
    got = np.asarray(got, f64).reshape(-1, 2)
    bad = []
    for i, t in enumerate(terms):
        n = len(t)
        for k, tt in enumerate((t, t * t)):
            dev = abs(math.fsum(list(tt) + [-got[i, k]]))
            if not dev <= n * 2.0 ** -53 * math.fsum(np.abs(tt)):
                bad.append((i, k))
    return bad


def finish(axes, n1, s1, n2, s2, registration_error=0.0, min_count=4):
    """-> (distance, lod float64 (m,), significant uint8 (m,))."""
    d = _f32(axes, (-1, 3)).astype(f64)
    n1, n2 = np.asarray(n1, np.int32), np.asarray(n2, np.int32)
    s1, s2 = np.asarray(s1, f64).reshape(-1, 2), np.asarray(s2, f64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ok = np.isfinite(d).all(1) & (dd != 0.0) & (n1 >= min_count) & (n2 >= min_count)
        mean, var, cnt = [], [], []
        for n, s in ((n1, s1), (n2, s2)):
            k = n.astype(f64)
            v = (s[:, 1] - (s[:, 0] * s[:, 0]) / k) / (k - 1.0)
            mean.append(s[:, 0] / k)
            var.append(np.where(v > 0.0, v, 0.0) / dd)
            cnt.append(k)
        distance = (mean[1] - mean[0]) / np.sqrt(dd)
        lod = 1.96 * (np.sqrt(var[0] / cnt[0] + var[1] / cnt[1]) + f64(registration_error))
        sig = np.abs(distance) > lod
    return np.where(ok, distance, np.nan), np.where(ok, lod, np.nan), (sig & ok).astype(np.uint8)
