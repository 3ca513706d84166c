"""Brute-force NumPy restatement of k nearest neighbours (include/pcgx.h, pcgx_kdtree_knearest; csrc/knearest.hip).

No reference counterpart exists: this is the contract itself.  For query q, k and B = max_range^2 (float32):
  the k points p with the smallest (DistSq(p, q), id), lexicographic, among those with DistSq < B, ascending;
  DistSq is the reference's float32 (dx*dx + dy*dy) + dz*dz.  Slots past the count are {-1, B}.
Deleted points (`exclude`) are nobody's neighbour.  Non-finite queries find nothing (no DistSq of theirs is < B)."""
import numpy as np


def dist_sq_f32(points, q):
    """DistSq of every point to q in the reference's float32 expression (no fused multiply-add)."""
    p = np.asarray(points, np.float32)
    q = np.asarray(q, np.float32)
    dx = p[:, 0] - q[0]
    dy = p[:, 1] - q[1]
    dz = p[:, 2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def knearest_one(points, q, k, max_range, exclude=None):
    """(ids int64[c], dsq float32[c]) for one query, c <= k: np.lexsort((id, dsq)) of the admissible points."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    bound = np.float32(max_range) * np.float32(max_range)
    d = dist_sq_f32(points, q)
    ok = d < bound
    if exclude is not None:
        ok[np.asarray(exclude, np.int64)] = False
    ids = np.nonzero(ok)[0]
    order = np.lexsort((ids, d[ids]))[:k]
    return ids[order].astype(np.int64), d[ids][order]


def knearest(points, queries, k, max_range, exclude=None, chunk=1 << 24):
    """-> (ids int64 (m, k), dsq float32 (m, k), counts int32 (m,)) for every query, the layout of
    KDTree.KNearestBatch.  Vectorised over queries with 64-bit keys bits(dsq) << 32 | id (dsq >= 0: the bits order as
    the floats), which order exactly as np.lexsort((id, dsq))."""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    Q = np.asarray(queries, np.float32).reshape(-1, 3)
    n, m = len(P), len(Q)
    bound = np.float32(max_range) * np.float32(max_range)
    ids = np.full((m, k), -1, np.int64)
    dsq = np.full((m, k), bound, np.float32)
    counts = np.zeros(m, np.int32)
    keep = np.ones(n, bool)
    if exclude is not None:
        keep[np.asarray(exclude, np.int64)] = False
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    step = max(1, chunk // max(n, 1))
    pid = np.arange(n, dtype=np.uint64)
    for a in range(0, m, step):
        q = Q[a:a + step]
        dx = P[None, :, 0] - q[:, None, 0]
        dy = P[None, :, 1] - q[:, None, 1]
        dz = P[None, :, 2] - q[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        ok = (d < bound) & keep[None, :]
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | pid[None, :]
        key = np.where(ok, key, none)
        kk = min(k, n)
        if kk < n:
            key = np.partition(key, kk - 1, axis=1)[:, :kk]
        key = np.sort(key, axis=1)[:, :kk]
        valid = key != none
        c = valid.sum(1).astype(np.int32)
        counts[a:a + step] = c
        got_ids = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
        got_d = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
        blk_i = ids[a:a + step, :kk]
        blk_d = dsq[a:a + step, :kk]
        blk_i[valid] = got_ids[valid]
        blk_d[valid] = got_d[valid]
    return ids, dsq, counts


def range_sorted(points, q, max_range, exclude=None):
    """Range's set for one query ordered by (dsq, id): (ids, dsq) -- for the prefix comparisons."""
    return knearest_one(points, q, len(points), max_range, exclude)
