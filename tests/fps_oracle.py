"""NumPy restatement of farthest-point sampling (include/pcgx.h, "farthest-point sampling"): the contract the GPU tests
compare with by array_equal.  Not a test module.

    E        the points that are not deleted and whose x, y, z are all finite
    DistSq   float32, (dx dx + dy dy) + dz dz of d = p - q, each operation rounded once
    d        the running minimum of DistSq to the picks so far, STRICT update nd < d; the owner is the pick that last
             lowered it (the earliest of the nearest picks)
    pick     the unpicked point of E with the largest d, the first index among equals
"""
import numpy as np

f32 = np.float32


def dist_sq(P, s):
    """float32 DistSq of every row of P (n, 3) float32 to the point s (3,) float32, in the contract's order."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = P - s
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def eligible(P, deleted=None):
    P = np.asarray(P, f32).reshape(-1, 3)
    e = np.isfinite(P).all(axis=1)
    if deleted is not None:
        e &= ~np.asarray(deleted, bool)
    return e


def fps(P, count, start=-1, deleted=None):
    """-> dict(ids int64 (count,) padded with -1, n_ids, dist_sq float32 (count,) padded with -1, cover_sq float32,
    owner int64 (n,), d float32 (n,) the final running minimum (+inf where nothing was picked), picked bool (n,))."""
    P = np.ascontiguousarray(np.asarray(P, f32).reshape(-1, 3))
    n = len(P)
    E = eligible(P, deleted)
    ids = np.full(count, -1, np.int64)
    dsq = np.full(count, -1.0, f32)
    owner = np.full(n, -1, np.int64)
    d = np.full(n, np.inf, f32)
    cand = E.copy()
    if start >= 0:
        assert E[start], "start must be eligible"
    k = 0
    cur, cur_d = (int(start), f32(np.inf)) if start >= 0 else ((int(np.flatnonzero(E)[0]), f32(np.inf)) if E.any() else (-1, f32(-1)))
    key = np.empty(n, f32)
    while k < count and cur >= 0:
        ids[k], dsq[k] = cur, cur_d
        k += 1
        nd = dist_sq(P, P[cur])
        upd = E & (nd < d)
        d[upd] = nd[upd]
        owner[upd] = cur
        cand[cur] = False
        if not cand.any():
            cur = -1
            break
        key[:] = -1.0
        key[cand] = d[cand]
        cur = int(np.argmax(key))  # the first index among equals: the smallest id
        cur_d = d[cur]
    cover = cur_d if cur >= 0 and k > 0 else f32(-1.0)
    return dict(ids=ids, n_ids=k, dist_sq=dsq, cover_sq=f32(cover), owner=owner, d=d, picked=E & ~cand)


def bits(a):
    return np.asarray(a, f32).reshape(-1).view(np.uint32)
