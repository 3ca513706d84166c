"""float64 NumPy restatement of surface-normal estimation (include/pcgx.h, pcgx_kdtree_normals; csrc/normals.hip).

No reference counterpart exists (pcgol has no normal estimation): this is the contract itself.  For query q, radius
r, viewpoint v and min_neighbors (below 3 counts as 3):
  N(q)  = the points p with DistSq(p, q) < r*r, DistSq the reference's float32 (dx*dx + dy*dy) + dz*dz;
  count = |N(q)|; fewer than min_neighbors, or all of N(q) at one place: normal 0, curvature NaN;
  else, with d = p - q in float64: C = sum d d^T / count - mean mean^T, eigenvalues l0 <= l1 <= l2,
  normal = unit eigenvector of l0, negated if normal . (v - q) < 0; curvature = max(l0, 0) / (l0 + l1 + l2).
Neighbour lists come from brute_force_lists (small clouds) or from the library's Range batch (range_lists), which
tests/test_gpu_kdtree.py pins to the C oracle."""
import numpy as np


def dist_sq_f32(points, q):
    """DistSq of every point to q in the reference's float32 expression (no fused multiply-add)."""
    p = np.asarray(points, np.float32)
    q = np.asarray(q, np.float32)
    dx = p[:, 0] - q[0]
    dy = p[:, 1] - q[1]
    dz = p[:, 2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def brute_force_lists(points, queries, radius):
    """(offsets int64[m+1], ids int64[total]) of N(q) for every query, by looking at every point."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    queries = np.asarray(queries, np.float32).reshape(-1, 3)
    bound = np.float32(radius) * np.float32(radius)
    lists = [np.nonzero(dist_sq_f32(points, q) < bound)[0] for q in queries]
    offs = np.zeros(len(queries) + 1, np.int64)
    np.cumsum([len(a) for a in lists], out=offs[1:])
    ids = np.concatenate(lists).astype(np.int64) if lists else np.zeros(0, np.int64)
    return offs, ids


def range_lists(tree, queries, radius):
    """The same lists from KDTree.RangeBatch (pcgx_kdtree_range_count / _fill)."""
    offs, ids, _ = tree.RangeBatch(np.asarray(queries, np.float32).reshape(-1, 3), radius)
    return offs, ids


def normals_from_lists(points, queries, offs, ids, viewpoint=(0.0, 0.0, 0.0), min_neighbors=3, chunk=1 << 22):
    """-> dict(normals f32 (m,3), curvature f32 (m,), counts i32 (m,), lam f64 (m,3) ascending (NaN where
    degenerate), degenerate bool (m,))."""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    Q = np.asarray(queries, np.float32).reshape(-1, 3)
    offs = np.asarray(offs, np.int64)
    ids = np.asarray(ids, np.int64)
    m = len(Q)
    mn = max(int(min_neighbors), 3)
    v = np.asarray(viewpoint, np.float32).astype(np.float64)
    counts = np.diff(offs)
    normals = np.zeros((m, 3), np.float32)
    curv = np.full(m, np.nan, np.float32)
    lam = np.full((m, 3), np.nan)
    degen = np.ones(m, bool)
    a = 0
    while a < m:  # query chunks of at most `chunk` neighbours (or one query)
        b = max(a + 1, min(m, int(np.searchsorted(offs, offs[a] + chunk, side="right")) - 1))
        sel = np.arange(a, b)[counts[a:b] >= mn]
        qall = np.repeat(np.arange(a, b), counts[a:b])
        seg = np.arange(offs[a], offs[b])[counts[qall] >= mn]  # the rows of the selected queries, back to back
        a = b
        if len(sel) == 0:
            continue
        loc = np.zeros(len(sel), np.int64)
        np.cumsum(counts[sel][:-1], out=loc[1:])
        qi = np.repeat(sel, counts[sel])
        pj = P[ids[seg]]
        lo = np.minimum.reduceat(pj, loc, axis=0)
        hi = np.maximum.reduceat(pj, loc, axis=0)
        spread = np.any(lo != hi, axis=1)
        d = pj.astype(np.float64) - Q[qi].astype(np.float64)
        c = counts[sel].astype(np.float64)
        s1 = np.add.reduceat(d, loc, axis=0)
        s2 = np.add.reduceat(d[:, :, None] * d[:, None, :], loc, axis=0)
        mean = s1 / c[:, None]
        C = s2 / c[:, None, None] - mean[:, :, None] * mean[:, None, :]
        tr = np.trace(C, axis1=1, axis2=2)
        ok = spread & (tr > 0)
        if not np.any(ok):
            continue
        rows = sel[ok]
        w, V = np.linalg.eigh(C[ok])
        n = V[:, :, 0]
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        dot = np.sum(n * (v[None, :] - Q[rows].astype(np.float64)), axis=1)
        n[dot < 0] *= -1.0
        normals[rows] = n.astype(np.float32)
        curv[rows] = (np.maximum(w[:, 0], 0.0) / np.sum(w, axis=1)).astype(np.float32)
        lam[rows] = w
        degen[rows] = False
    return dict(normals=normals, curvature=curv, counts=counts.astype(np.int32), lam=lam, degenerate=degen)


def normals(points, queries, radius, viewpoint=(0.0, 0.0, 0.0), min_neighbors=3):
    """Brute force end to end (small clouds)."""
    offs, ids = brute_force_lists(points, queries, radius)
    return normals_from_lists(points, queries, offs, ids, viewpoint, min_neighbors)
