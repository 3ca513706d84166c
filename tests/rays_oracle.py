"""The contract of the ray queries (include/pcgx.h, "ray queries") restated in NumPy float64, brute force over all
(ray, point) pairs.  float64 from the float32 inputs widened, the operation order as written there, every product and sum
rounded once (NumPy fuses nothing), no square root and no division in what a result is made of.  The box clip
(csrc/ray_terms.h, ray_clip) is restated too: it divides, in IEEE float64."""
import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -20
CHUNK = 32  # rays per block of the brute force


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, f32)
    return a if shape is None else a.reshape(shape)


def bounds(nr, s_min=None, s_max=None):
    """s_min, s_max as float32 (nr,) arrays: None is 0 and +inf."""
    lo = np.zeros(nr, f32) if s_min is None else np.broadcast_to(np.asarray(s_min, f32), (nr,)).copy()
    hi = np.full(nr, np.inf, f32) if s_max is None else np.broadcast_to(np.asarray(s_max, f32), (nr,)).copy()
    return lo, hi


def ray_terms(o, d, s_min, s_max, rho):
    """dd, rr dd, s_min dd, s_max dd, usable -- per ray."""
    o, d = _f32(o, (-1, 3)).astype(f64), _f32(d, (-1, 3)).astype(f64)
    lo, hi = bounds(len(o), s_min, s_max)
    with np.errstate(all="ignore"):
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        rr = f64(f32(rho)) * f64(f32(rho))
        rrdd = rr * dd
        a_lo, a_hi = lo.astype(f64) * dd, hi.astype(f64) * dd
        usable = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (dd != 0.0) & ~np.isnan(lo) & ~np.isnan(hi) & ~(lo > hi)
    return dd, rrdd, a_lo, a_hi, usable


def pair_terms(o, d, p):
    """a and cc of every (ray, point) pair: (nr, n) float64 each."""
    o, d, p = (_f32(x, (-1, 3)).astype(f64) for x in (o, d, p))
    with np.errstate(all="ignore"):
        wx, wy, wz = (p[None, :, k] - o[:, None, k] for k in range(3))
        dx, dy, dz = (d[:, None, k] for k in range(3))
        a = (wx * dx + wy * dy) + wz * dz
        cx, cy, cz = wy * dz - wz * dy, wz * dx - wx * dz, wx * dy - wy * dx
        cc = (cx * cx + cy * cy) + cz * cz
    return a, cc


def members(points, o, d, s_min, s_max, rho, deleted=None):
    """(member (nr, n) bool, a, cc)."""
    points = _f32(points, (-1, 3))
    dd, rrdd, a_lo, a_hi, usable = ray_terms(o, d, s_min, s_max, rho)
    a, cc = pair_terms(o, d, points)
    live = np.isfinite(points).all(1)
    if deleted is not None and len(deleted):
        live = live.copy()
        live[np.asarray(deleted, np.int64)] = False
    with np.errstate(all="ignore"):
        m = (cc <= rrdd[:, None]) & (a_lo[:, None] <= a) & (a <= a_hi[:, None])
    return m & usable[:, None] & live[None, :], a, cc


def beats(a, i, b, j):
    """Does the hit (a, id i) beat (b, id j)?  An id < 0 is no hit."""
    if i < 0:
        return False
    if j < 0:
        return True
    return bool(a < b or (a == b and i < j))


def _blocks(points, o, d, s_min, s_max, rho, deleted):
    o, d = _f32(o, (-1, 3)), _f32(d, (-1, 3))
    lo, hi = bounds(len(o), s_min, s_max)
    for f in range(0, len(o), CHUNK):
        e = min(f + CHUNK, len(o))
        yield f, e, members(points, o[f:e], d[f:e], lo[f:e], hi[f:e], rho, deleted)


def query(points, o, d, rho, s_min=None, s_max=None, deleted=None, ranks=1):
    """One pass over all pairs -> (hits, counts).  hits[k] = (ids int64 (-1: none), along = a, off_sq = cc (0 for a
    miss)) of each ray's member number k in the order (a, id): hits[0] is the first hit -- the member with the smallest
    a, a tie going to the smallest id --, hits[1] what is first once the first hits are gone.  counts int32 (n,): one
    for every (ray, member) pair."""
    nr, n = len(_f32(o, (-1, 3))), len(_f32(points, (-1, 3)))
    hits = [(np.full(nr, -1, np.int64), np.zeros(nr, f64), np.zeros(nr, f64)) for _ in range(ranks)]
    counts = np.zeros(n, np.int64)
    for f, e, (m, a, cc) in _blocks(points, o, d, s_min, s_max, rho, deleted):
        if n == 0:
            continue
        counts += m.sum(0)
        key = np.where(m, a, np.inf)
        rows = np.arange(e - f)
        for ids, along, off in hits:
            j = np.argmin(key, axis=1)  # (argmin takes the first, i.e. the smallest id, of equal keys)
            hit = m[rows, j]
            ids[f:e] = np.where(hit, j, -1)
            along[f:e] = np.where(hit, a[rows, j], 0.0)
            off[f:e] = np.where(hit, cc[rows, j], 0.0)
            key[rows, j] = np.inf
            m[rows, j] = False
    return hits, counts.astype(np.int32)


def raycast(points, o, d, rho, s_min=None, s_max=None, deleted=None, rank=0):
    """(ids, along, off_sq) of the first hits; rank = 1: of the second members."""
    return query(points, o, d, rho, s_min, s_max, deleted, rank + 1)[0][rank]


def pierce(points, o, d, rho, s_min=None, s_max=None, deleted=None):
    return query(points, o, d, rho, s_min, s_max, deleted)[1]


def finite_box(points):
    """(lo (3,), hi (3,), any) float32 over the points with three finite coordinates."""
    points = _f32(points, (-1, 3))
    fin = points[np.isfinite(points).all(1)]
    if len(fin) == 0:
        return np.zeros(3, f32), np.zeros(3, f32), False
    return fin.min(0), fin.max(0), True


def clip(o, d, s_min, s_max, rho, lo, hi, any_point=True):
    """ray_clip per ray: (ok bool, a0, a1) -- the range of a = s dd inside the box [lo, hi] inflated by
    pad = rho (1 + 2^-20) + 2^-20 M, M the largest magnitude among o, lo and hi, cut to [s_min dd, s_max dd]."""
    o64, d64 = _f32(o, (-1, 3)).astype(f64), _f32(d, (-1, 3)).astype(f64)
    nr = len(o64)
    dd, _, a_lo, a_hi, usable = ray_terms(o, d, s_min, s_max, rho)
    lo64, hi64 = _f32(lo).astype(f64), _f32(hi).astype(f64)
    ok, a0, a1 = np.zeros(nr, bool), np.zeros(nr, f64), np.zeros(nr, f64)
    box_m = max(np.abs(lo64).max(), np.abs(hi64).max())
    for i in range(nr):
        if not (usable[i] and any_point):
            continue
        mag = max(np.abs(o64[i]).max(), box_m)
        pad = f64(f32(rho)) * (1.0 + U) + U * mag
        s0, s1, out = -np.inf, np.inf, False
        for k in range(3):
            f0, f1 = lo64[k] - pad, hi64[k] + pad
            if d64[i, k] == 0.0:
                if o64[i, k] < f0 or o64[i, k] > f1:
                    out = True
                    break
                continue
            t0, t1 = (f0 - o64[i, k]) / d64[i, k], (f1 - o64[i, k]) / d64[i, k]
            s0, s1 = max(s0, min(t0, t1)), min(s1, max(t0, t1))
        if out:
            continue
        a0[i], a1[i] = max(s0 * dd[i], a_lo[i]), min(s1 * dd[i], a_hi[i])
        ok[i] = a0[i] <= a1[i]
    return ok, a0, a1
