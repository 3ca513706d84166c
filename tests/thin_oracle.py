"""NumPy oracle of minimum-distance subsampling (include/pcgx.h, "minimum-distance subsampling"; csrc/thin.hip,
csrc/thin_terms.h), restated.  NumPy only.

  neighbours   N(i) = {j : (dx dx + dy dy) + dz dz < f32(r) f32(r)}, all float32, strict, over the live points; a deleted
               point or one with a NaN / infinite coordinate is in no list, not its own either.
  eligible     i in N(i), and in score mode score[i] is no NaN.
  priority     hash mode: the smaller (shape_mix(seed, id) << 32) | id first; score mode: j before i iff
               score[j] > score[i] or (score[j] == score[i] and j < i).  rank[i] = i's place in that order, -1 outside E.
  greedy       visit E in priority order, keep a point iff no kept point is in its list.
  rounds       the parallel rule: from the states as the round before left them, an undecided i is DROPPED if a
               neighbour before it is KEPT, else KEPT if no neighbour before it is UNDECIDED, else stays.
  owner        a kept point itself; a dropped point the kept neighbour of the smallest (DistSq, id); else -1.

Neighbour lists come in two forms behind one interface (n, of(i) -> the ids of N(i), in any order): Lists over CSR arrays
(brute_lists; keypoints_oracle.brute_lists gives the same arrays), and SiteLists, one list per DISTINCT position found
through a cell grid -- heaps of thousands of coincident points share one list instead of holding millions of pairs."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

f32, u32, u64 = np.float32, np.uint32, np.uint64
UNDECIDED, KEPT, DROPPED, INELIGIBLE = 0, 1, 2, 3


def shape_mix(seed, ids):
    """csrc/shape_terms.h's shape_mix(seed, id) in uint32 arithmetic -> uint32 array"""
    with np.errstate(over="ignore"):
        x = u32(seed) ^ (np.asarray(ids).astype(u32) * u32(0x9E3779B1))
        x ^= x >> u32(16)
        x *= u32(0x85EBCA6B)
        x ^= x >> u32(13)
        x *= u32(0xC2B2AE35)
        x ^= x >> u32(16)
    return x


def hash_key(seed, ids):
    ids = np.asarray(ids)
    return (shape_mix(seed, ids).astype(u64) << u64(32)) | ids.astype(u64)


def dist_sq(p, q):
    """the reference's float32 DistSq of every row of p to q"""
    p = np.asarray(p, f32).reshape(-1, 3)
    q = np.asarray(q, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = p[:, 0] - q[0], p[:, 1] - q[1], p[:, 2] - q[2]
        return (dx * dx + dy * dy) + dz * dz


def live_points(points, deleted=None):
    p = np.array(points, f32).reshape(-1, 3)
    if deleted is not None and len(deleted):
        p[np.asarray(deleted, np.int64)] = np.nan  # never DistSq < bound: nobody's neighbour, not its own either
    return p


class Lists:
    """N(i) for every id from CSR arrays (offsets [n + 1], ids ascending within a list)"""

    def __init__(self, offs, ids):
        self.offs, self.ids = np.asarray(offs, np.int64), np.asarray(ids, np.int64)
        self.n = len(self.offs) - 1

    def of(self, i):
        return self.ids[self.offs[i]:self.offs[i + 1]]


def brute_lists(points, radius, deleted=None):
    """Lists by looking at every pair"""
    p = live_points(points, deleted)
    bound = f32(radius) * f32(radius)
    with np.errstate(invalid="ignore"):
        rows = [np.nonzero(dist_sq(p, q) < bound)[0] for q in p]
    offs = np.zeros(len(p) + 1, np.int64)
    np.cumsum([len(a) for a in rows], out=offs[1:])
    return Lists(offs, np.concatenate(rows) if rows else np.zeros(0, np.int64))


class SiteLists:
    """N(i) = the members of the sites within the bound of i's site (in no particular order).  site[i]: i's site, -1 for
    a point that is in no list; the members of site s: m_ids[m_offs[s]:m_offs[s + 1]]; the sites within the bound of s
    (s itself among them): near[n_offs[s]:n_offs[s + 1]]."""

    def __init__(self, n, site, m_offs, m_ids, n_offs, near):
        self.n, self.site, self.m_offs, self.m_ids, self.n_offs, self.near = n, site, m_offs, m_ids, n_offs, near

    def of(self, i):
        s = int(self.site[i])
        if s < 0:
            return np.zeros(0, np.int64)
        t = self.near[self.n_offs[s]:self.n_offs[s + 1]]
        lo = self.m_offs[t]
        cnt = self.m_offs[t + 1] - lo
        if cnt.sum() == len(t):
            return self.m_ids[lo]
        return self.m_ids[np.repeat(lo - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(cnt.sum())]

    def without(self, deleted):
        """the lists of the same cloud after the ids `deleted` have left it (a site may be left without members)"""
        site = self.site.copy()
        site[np.asarray(deleted, np.int64)] = -1
        stay = site[self.m_ids] >= 0
        sites = len(self.m_offs) - 1
        of_slot = np.repeat(np.arange(sites), np.diff(self.m_offs))
        m_offs = np.concatenate([[0], np.cumsum(np.bincount(of_slot[stay], minlength=sites))]).astype(np.int64)
        return SiteLists(self.n, site, m_offs, self.m_ids[stay], self.n_offs, self.near)


def site_lists(points, radius, deleted=None):
    """SiteLists through a grid of cells a little wider than the radius: the candidates of a site are the sites of the
    27 cells round its own, the test is the exact float32 one.  (A pair inside the float32 bound is closer than
    radius (1 + 1e-6), so no member lies beyond the neighbouring cells.)"""
    p = live_points(points, deleted)
    n = len(p)
    bound = f32(radius) * f32(radius)
    ok = np.isfinite(p).all(axis=1)
    site = np.full(n, -1, np.int64)
    if not ok.any() or not bound > 0:
        z = np.zeros(1, np.int64)
        return SiteLists(n, site, z, z[:0], z, z[:0])
    sel = np.nonzero(ok)[0]
    U, inv = np.unique(p[sel], axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    site[sel] = inv
    order = np.argsort(inv, kind="stable")
    cuts = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(U)))])
    m_ids = sel[order]
    edge = float(radius) * 1.001
    c = np.floor((U.astype(np.float64) - U.astype(np.float64).min(axis=0)) / edge).astype(np.int64) + 1
    dims = c.max(axis=0) + 2
    assert float(dims[0]) * float(dims[1]) * float(dims[2]) < 2.0 ** 62
    key = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    by_key = np.argsort(key, kind="stable")
    skey = key[by_key]
    pa, pb = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            want = key + (dz * dims[1] + dy) * dims[0]  # the three cells x - 1 .. x + 1 are one run of keys
            lo, hi = np.searchsorted(skey, want - 1, "left"), np.searchsorted(skey, want + 1, "right")
            cnt = hi - lo
            a = np.repeat(np.arange(len(U)), cnt)
            b = by_key[np.repeat(lo - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(cnt.sum())]
            d = U[b] - U[a]
            inside = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] < bound
            pa.append(a[inside])
            pb.append(b[inside])
    pa, pb = np.concatenate(pa), np.concatenate(pb)
    o = np.argsort(pa, kind="stable")
    pa, pb = pa[o], pb[o]
    ncuts = np.concatenate([[0], np.cumsum(np.bincount(pa, minlength=len(U)))])
    return SiteLists(n, site, cuts.astype(np.int64), m_ids, ncuts.astype(np.int64), pb)


def eligible(lists, score=None):
    """bool [n]: the point is in its own list, and its score (where there is one) is no NaN"""
    if isinstance(lists, SiteLists):
        e = lists.site >= 0  # (a site is within the bound of itself: 0 < bound)
    else:
        e = np.array([bool(np.any(lists.of(i) == i)) for i in range(lists.n)], bool)
    if score is not None:
        e &= ~np.isnan(np.asarray(score, f32).reshape(-1))
    return e


def priority_order(elig, seed=0, score=None):
    """the ids of E, the first in priority first"""
    ids = np.nonzero(elig)[0].astype(np.int64)
    if score is None:
        return ids[np.argsort(hash_key(seed, ids), kind="stable")]
    s = np.asarray(score, f32).reshape(-1)[ids] + f32(0.0)  # (-0 + 0 == +0: the two zeros tie)
    return ids[np.lexsort((ids, -s.astype(np.float64)))]


def rank_of(order, n):
    """rank[i] = i's place in the order, -1 outside it"""
    rank = np.full(n, -1, np.int64)
    rank[order] = np.arange(len(order))
    return rank


def greedy(lists, order):
    """sequential selection -> kept mask [n]"""
    kept = np.zeros(lists.n, bool)
    for i in order:
        if not kept[lists.of(i)].any():
            kept[i] = True
    return kept


def rounds(lists, rank, R=None):
    """the round rule -> (states after each round [(n,) uint8 ...], undecided counts after each round).  R = None: to
    completion."""
    n = lists.n
    state = np.where(rank >= 0, UNDECIDED, INELIGIBLE).astype(np.uint8)
    states, history = [], []
    while (R is None and (state == UNDECIDED).any()) or (R is not None and len(states) < R):
        new = state.copy()
        for i in np.nonzero(state == UNDECIDED)[0]:
            nb = lists.of(i)
            before = nb[(rank[nb] >= 0) & (rank[nb] < rank[i])]
            sb = state[before]
            if (sb == KEPT).any():
                new[i] = DROPPED
            elif not (sb == UNDECIDED).any():
                new[i] = KEPT
        state = new
        states.append(state)
        history.append(int((state == UNDECIDED).sum()))
    return states, history


def owner(points, lists, kept, elig, deleted=None):
    """int64 [n]: a kept point itself, a dropped point of E the kept neighbour of the smallest (DistSq, id), else -1.
    Over SiteLists kept point by kept point, ids ascending (the float32 DistSq is symmetric bit for bit, so k's list is the set of
    points that have k in theirs): a later one takes a point over only with a strictly smaller DistSq."""
    p = live_points(points, deleted)
    if not isinstance(lists, SiteLists):  # lists as given (they may come from a handle's own Range): point by point
        out = np.full(lists.n, -1, np.int64)
        for i in np.nonzero(elig)[0]:
            nb = lists.of(i)
            nb = nb[kept[nb]]
            out[i] = i if kept[i] else nb[np.lexsort((nb, dist_sq(p[nb], p[i])))[0]]
        return out
    best_d = np.full(lists.n, np.inf, f32)
    best = np.full(lists.n, -1, np.int64)
    for k in np.nonzero(kept)[0]:
        nb = lists.of(k)
        d = dist_sq(p[nb], p[k])
        take = d < best_d[nb]
        best_d[nb[take]] = d[take]
        best[nb[take]] = k
    assert np.all(best[elig] >= 0) and np.array_equal(best[kept], np.nonzero(kept)[0])
    return np.where(elig, best, -1)


def thin(points, radius, seed=0, score=None, deleted=None, lists=None):
    """the whole contract -> (ids int64 ascending, owner int64 [n], lists)"""
    if lists is None:
        lists = site_lists(points, radius, deleted)
    e = eligible(lists, score)
    kept = greedy(lists, priority_order(e, seed, score))
    return np.nonzero(kept)[0].astype(np.int64), owner(points, lists, kept, e, deleted), lists
