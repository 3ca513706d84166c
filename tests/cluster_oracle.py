"""NumPy oracle of cluster extraction: the contract of include/pcgx.h ("clusters"), restated.  NumPy only.

Neighbourhood  N(i) = the points p with DistSq(p, point i) < radius^2, DistSq the float32 expression
               (dx dx + dy dy) + dz dz.  A deleted point is given as NaN coordinates: nobody's neighbour.
Usable point   i in N(i) (finite coordinates); with normals: the three components finite and not all zero; with
               curvature: curvature[i] <= max_curvature (a NaN fails).
Edge           both usable, j in N(i), and with normals c = (nx_i nx_j + ny_i ny_j) + nz_i nz_j in float64 from the
               float32 components satisfies c >= min_cos (oriented) or |c| >= min_cos.
Clusters       the connected components of the usable points with max(min_size, 1) <= size (<= max_size unless 0),
               numbered by decreasing size, equal sizes by the smallest member id.
Outputs        labels [n] (-1: no cluster), C, sizes [n] (zero padded), ids [n] (cluster by cluster, ascending ids in
               each, -1 padded).

Pairs come from brute force over float32 differences in blocks of sites.  Coincident usable points whose normals have
equal bits (and agree with themselves) are one site first, so a heap of thousands of copies stays cheap.  The sites
are sorted by x and a block is compared with the sites whose x lies within 1.01 radius + the block's extent only: a
pair with DistSq < radius^2 has dx dx <= DistSq, so |dx| < radius (1 + 2^-23), far inside the window.  Components: min-label
propagation over the pairs with pointer jumping, as _components_reference in tests/test_gpu_radius_edges.py."""
import numpy as np

f32 = np.float32
BLOCK = 512


def dist_sq(a, b):
    """the reference's float32 DistSq, broadcasting over (..., 3)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def normal_ok(normals):
    n = np.asarray(normals, f32).reshape(-1, 3)
    return np.all(np.isfinite(n), axis=1) & ~np.all(n == 0, axis=1)


def usable(pts, radius, normals=None, curvature=None, max_curvature=0.0):
    pts = np.asarray(pts, f32).reshape(-1, 3)
    bound = f32(radius) * f32(radius)
    with np.errstate(invalid="ignore"):
        u = dist_sq(pts, pts) < bound
        if normals is not None:
            u &= normal_ok(normals)
        if curvature is not None:
            u &= np.asarray(curvature, f32).reshape(-1) <= f32(max_curvature)
    return u


def normals_agree(ni, nj, min_cos, oriented):
    """the edge predicate on rows of float32 normals (both points usable)"""
    a, b = np.asarray(ni, f32).astype(np.float64), np.asarray(nj, f32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        c = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
        return (c if oriented else np.abs(c)) >= np.float64(f32(min_cos))


def size_kept(size, min_size, max_size):
    size = np.asarray(size, np.int64)
    keep = size >= max(int(min_size), 1)
    if max_size > 0:
        keep &= size <= int(max_size)
    return keep


def site_pairs(sp, radius):
    """(a, b): every ordered pair a != b of rows of sp (finite float32 points) with DistSq < radius^2"""
    bound = f32(radius) * f32(radius)
    order = np.argsort(sp[:, 0], kind="stable")
    s = sp[order]
    xs = s[:, 0].astype(np.float64)
    reach = 1.01 * float(f32(radius))
    a_list, b_list = [], []
    for s0 in range(0, len(s), BLOCK):
        blk = s[s0:s0 + BLOCK]
        lo = np.searchsorted(xs, xs[s0] - reach, side="left")
        hi = np.searchsorted(xs, xs[min(s0 + BLOCK, len(s)) - 1] + reach, side="right")
        d = dist_sq(blk[:, None, :], s[None, lo:hi, :])
        a, b = np.nonzero(d < bound)
        a, b = a + s0, b + lo
        keep = a != b
        a_list.append(order[a[keep]])
        b_list.append(order[b[keep]])
    if not a_list:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(a_list), np.concatenate(b_list)


def components(m, a, b):
    """root[k] = the smallest member of k's component of the graph on m vertices with edges (a, b)"""
    parent = np.arange(m)
    while True:
        low = np.minimum(parent[a], parent[b])
        new = parent.copy()
        np.minimum.at(new, parent[a], low)
        np.minimum.at(new, parent[b], low)
        while True:  # pointer jumping
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, parent):
            return parent
        parent = new


def rank_and_group(n, name, min_size=1, max_size=0):
    """name [n]: the smallest id of every point's component, -1 for an unusable point -> (labels, C, sizes, ids)"""
    name = np.asarray(name, np.int64)
    labels = np.full(n, -1, np.int64)
    sizes = np.zeros(n, np.int64)
    ids = np.full(n, -1, np.int64)
    seeds, count = np.unique(name[name >= 0], return_counts=True)
    keep = size_kept(count, min_size, max_size)
    seeds, count = seeds[keep], count[keep]
    order = np.lexsort((seeds, -count))  # by decreasing size, equal sizes by the smallest id
    seeds, count = seeds[order], count[order]
    c = len(seeds)
    if c:
        rank = np.full(n, -1, np.int64)
        rank[seeds] = np.arange(c)
        labels[name >= 0] = rank[name[name >= 0]]
        sizes[:c] = count
        members = np.nonzero(labels >= 0)[0]
        members = members[np.argsort(labels[members], kind="stable")]
        ids[:len(members)] = members
    return labels, c, sizes, ids


def names(pts, radius, normals=None, min_cos=0.0, oriented=False, curvature=None, max_curvature=0.0):
    """name[i] = the smallest id of i's component, -1 for an unusable point"""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    n = len(pts)
    nrm = None if normals is None else np.ascontiguousarray(normals, f32).reshape(-1, 3)
    u = usable(pts, radius, nrm, curvature, max_curvature)
    idx = np.nonzero(u)[0]
    name = np.full(n, -1, np.int64)
    if len(idx) == 0:
        return name
    key = pts[idx].view(np.uint32).astype(np.int64)
    if nrm is not None:
        own = normals_agree(nrm[idx], nrm[idx], min_cos, oriented)  # coincident copies join only if a normal agrees with itself
        apart = np.where(own, -1, idx)[:, None]
        key = np.concatenate([key, nrm[idx].view(np.uint32).astype(np.int64), apart], axis=1)
    _, first, site = np.unique(key, axis=0, return_index=True, return_inverse=True)
    site = site.reshape(-1)
    sp = pts[idx][first]
    a, b = site_pairs(sp, radius)
    if nrm is not None and len(a):
        sn = nrm[idx][first]
        ok = normals_agree(sn[a], sn[b], min_cos, oriented)
        a, b = a[ok], b[ok]
    root = components(len(sp), a, b)
    low = np.full(len(sp), n, np.int64)
    np.minimum.at(low, root[site], idx)
    name[idx] = low[root[site]]
    return name


def clusters(pts, radius, normals=None, min_cos=0.0, oriented=False, curvature=None, max_curvature=0.0, min_size=1,
             max_size=0):
    """-> (labels [n] int64, C, sizes [n] int64 zero padded, ids [n] int64 -1 padded)"""
    name = names(pts, radius, normals, min_cos, oriented, curvature, max_curvature)
    return rank_and_group(len(name), name, min_size, max_size)
