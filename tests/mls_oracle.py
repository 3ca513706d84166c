"""float64 NumPy restatement of moving-least-squares smoothing (include/pcgx.h, pcgx_kdtree_mls; csrc/mls.hip,
csrc/mls_terms.h).

No reference counterpart exists: this is the contract itself.  For query q, radius r, sigma, order, viewpoint v and
min_neighbors (below 3 counts as 3), over N(q) = the points with float32 DistSq(p, q) < r*r, count = |N(q)|:
  kind 0: count < min_neighbors, all of N(q) at one place, or trace C <= 0: the query's bits, normal 0;
  kind 1: d = p - q in float64, C = sum d d^T / count - mean mean^T, eigenvectors n, u, v of l0 <= l1 <= l2;
          d0 = (mean . n) n; position q + d0, normal n;
  kind 2 (order 2, count >= 6): e = d - d0, h = e . n, a = e . u / r, b = e . v / r, w = exp(-|e|^2 / sigma^2),
          B = (1, a, b, a^2, a b, b^2), M = sum w B B^T, g = sum w B h, Cholesky in that order (fails when sum w is not
          > 0 or a pivot s_k = M_kk - sum_j L_kj^2 is not > 1e-10 M_kk: kind 1), c = M^-1 g, |c0| > r: kind 1; else
          position q + d0 + c0 n, normal n - (c1 / r) u - (c2 / r) v normalised.
  Normals of kind 1 and 2 are negated where normal . (v - q) < 0; everything is rounded to float32 once.
Neighbour lists come from normals_oracle.brute_force_lists or range_lists.  `order_rng`: sum every list in an order
drawn from that generator instead of the given one (the tests bound what the order of summation can move)."""
import numpy as np

PIVOT_MIN = 1e-10
UNCHANGED, PLANE, POLY = 0, 1, 2


def cholesky_solve(M, g):
    """-> (c or None, pivot ratio): the contract's solve of the 6 x 6 system, pivots in the basis' order."""
    n = len(g)
    L = np.zeros((n, n))
    ratio = 1.0
    for j in range(n):
        mjj = M[j, j]
        if not mjj > 0.0:
            return None, 0.0
        s = mjj - float(np.dot(L[j, :j], L[j, :j]))
        ratio = min(ratio, s / mjj)
        if not s > PIVOT_MIN * mjj:
            return None, ratio
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            L[i, j] = (M[j, i] - float(np.dot(L[i, :j], L[j, :j]))) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (g[i] - float(np.dot(L[i, :i], y[:i]))) / L[i, i]
    c = np.zeros(n)
    for i in range(n - 1, -1, -1):
        c[i] = (y[i] - float(np.dot(L[i + 1:, i], c[i + 1:]))) / L[i, i]
    return c, ratio


def mls_from_lists(points, queries, offs, ids, radius, sigma=None, order=2, min_neighbors=3, viewpoint=(0.0, 0.0, 0.0),
                   order_rng=None):
    """-> dict(points f32 (m,3), normals f32 (m,3), kinds i32 (m,), counts i32 (m,), gap f64 (m,) = (l1 - l0) / l2
    (NaN for kind 0), pivot f64 (m,) = the pivot ratio (NaN where no solve was tried), c0 f64 (m,) (NaN where the solve
    was not tried or failed), points64, normals64: positions and normals before the rounding to float32)."""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    Q = np.asarray(queries, np.float32).reshape(-1, 3)
    offs = np.asarray(offs, np.int64)
    ids = np.asarray(ids, np.int64)
    m = len(Q)
    r = float(np.float32(radius))
    s = r if sigma is None else float(np.float32(sigma))
    mn = max(int(min_neighbors), 3)
    vp = np.asarray(viewpoint, np.float32).astype(np.float64)
    out_p = Q.copy()
    out_n = np.zeros((m, 3), np.float32)
    kinds = np.zeros(m, np.int32)
    counts = np.diff(offs).astype(np.int32)
    gap = np.full(m, np.nan)
    pivot = np.full(m, np.nan)
    c0 = np.full(m, np.nan)
    p64 = Q.astype(np.float64)
    n64 = np.zeros((m, 3))
    for i in range(m):
        if counts[i] < mn:
            continue
        nb = ids[offs[i]:offs[i + 1]]
        if order_rng is not None:
            nb = nb[order_rng.permutation(len(nb))]
        pj = P[nb]
        if np.all(pj.min(0) == pj.max(0)):
            continue
        q = Q[i].astype(np.float64)
        d = pj.astype(np.float64) - q
        mean = d.sum(0) / len(d)
        C = d.T @ d / len(d) - np.outer(mean, mean)
        if not np.trace(C) > 0.0:
            continue
        w, V = np.linalg.eigh(C)
        n, u, v = V[:, 0] / np.linalg.norm(V[:, 0]), V[:, 1], V[:, 2]
        gap[i] = (w[1] - w[0]) / w[2]
        d0 = np.dot(mean, n) * n
        kinds[i] = PLANE
        pos, nrm = q + d0, n
        if order == 2 and counts[i] >= 6:
            e = d - d0
            h = e @ n
            a = (e @ u) / r
            b = (e @ v) / r
            wt = np.exp(-np.sum(e * e, axis=1) / (s * s))
            B = np.stack([np.ones_like(a), a, b, a * a, a * b, b * b], axis=1)
            if wt.sum() > 0.0:
                c, pivot[i] = cholesky_solve((B * wt[:, None]).T @ B, (B * wt[:, None]).T @ h)
            else:
                c, pivot[i] = None, 0.0
            if c is not None:
                c0[i] = c[0]
                if not abs(c[0]) > r:
                    kinds[i] = POLY
                    pos = q + d0 + c[0] * n
                    nrm = n - (c[1] / r) * u - (c[2] / r) * v
                    nrm = nrm / np.linalg.norm(nrm)
        if np.dot(nrm, vp - q) < 0.0:
            nrm = -nrm
        p64[i], n64[i] = pos, nrm
        out_p[i] = pos.astype(np.float32)
        out_n[i] = nrm.astype(np.float32)
    return dict(points=out_p, normals=out_n, kinds=kinds, counts=counts, gap=gap, pivot=pivot, c0=c0, points64=p64,
                normals64=n64)


def mls(points, queries, radius, sigma=None, order=2, min_neighbors=3, viewpoint=(0.0, 0.0, 0.0), order_rng=None):
    """Brute force end to end (small clouds)."""
    import normals_oracle as NO
    offs, ids = NO.brute_force_lists(points, queries, radius)
    return mls_from_lists(points, queries, offs, ids, radius, sigma, order, min_neighbors, viewpoint, order_rng)


# ---------------------------------------------------------------------------------------------------------------
# What the GPU tests (tests/test_gpu_mls.py) and the host test of mls_terms.h ask of a result, stated once.

def good(ref):
    """The queries whose position and normal are compared: a polynomial was fitted, the plane's normal is well
    separated (gap >= 1e-3) and the solve well conditioned (pivot ratio >= 1e-6)."""
    return (ref["kinds"] == POLY) & (ref["gap"] >= 1e-3) & (ref["pivot"] >= 1e-6)


def fragile(ref, radius):
    """The queries whose kind may fall either way (1 or 2): the pivot ratio in (1e-12, 1e-8) round the threshold 1e-10
    -- the pivots depend on which u, v the eigen-solve returns --, or |c0| within 1e-6 radius of the radius."""
    r = float(np.float32(radius))
    p, c0 = ref["pivot"], ref["c0"]
    with np.errstate(invalid="ignore"):
        return ((p > 1e-12) & (p < 1e-8)) | (np.abs(np.abs(c0) - r) <= 1e-6 * r)


def position_tolerance(ref, radius):
    """Per coordinate: 2^-23 |oracle| (the one float32 rounding, doubled) + 1e-12 radius / pivot ratio (float64
    summation order and eigenvector noise amplified by the solve's conditioning); (m,3), NaN off the solved queries."""
    r = float(np.float32(radius))
    with np.errstate(divide="ignore"):  # (a pivot ratio of 0: a failed solve, never a good query)
        return 2.0 ** -23 * np.abs(ref["points"].astype(np.float64)) + (1e-12 * r / ref["pivot"])[:, None]


def check(got, ref, radius, what=""):
    """got = (points, normals, kinds, counts) against the oracle's `ref`: counts exact, kinds exact off the fragile
    queries (there 1 or 2), kind 0 the query's bits and a zero normal, positions within position_tolerance and normals
    within sin <= 1e-6 on the good queries.  -> the good mask."""
    points, normals, kinds, counts = got
    assert np.array_equal(counts, ref["counts"]), what
    fr = fragile(ref, radius)
    assert np.array_equal(kinds[~fr], ref["kinds"][~fr]), (what, np.nonzero(kinds != ref["kinds"])[0][:10])
    assert np.all((kinds[fr] == PLANE) | (kinds[fr] == POLY)), what
    assert not np.any(fr & (ref["kinds"] == UNCHANGED)), what
    z = ref["kinds"] == UNCHANGED
    assert np.array_equal(points[z].view(np.uint32), ref["points"][z].view(np.uint32)), what
    assert np.all(normals[z] == 0), what
    nz = ~z
    assert np.allclose(np.linalg.norm(normals[nz].astype(np.float64), axis=1), 1.0, atol=1e-6), what
    g = good(ref) & (kinds == POLY)
    assert np.array_equal(g, good(ref)) or np.all(fr[g != good(ref)]), what
    err = np.abs(points[g].astype(np.float64) - ref["points"][g].astype(np.float64))
    tol = position_tolerance(ref, radius)[g]
    print("%s: good %d of %d, worst position error / tolerance %.3g" % (what, int(g.sum()), len(kinds),
                                                                         float(np.max(err / tol, initial=0.0))))
    assert np.all(err <= tol), (what, float(np.max(err / tol)))
    a = normals[g].astype(np.float64)
    b = ref["normals"][g].astype(np.float64)
    sin = np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    print("%s: worst sin of the normals' angle %.3g" % (what, float(np.max(sin, initial=0.0))))
    assert np.max(sin, initial=0.0) <= 1e-6, (what, float(np.max(sin)))
    assert np.all(np.sum(a * b, axis=1) > 0), what  # (the same side: a good query's normal is far from perpendicular ...)
    return g


# ---------------------------------------------------------------------------------------------------------------
# Scenes shared by the CPU and the GPU tests.

def noisy_surface(n=3000, width=2.0, seed=21, noise=0.01, noise_seed=3):
    """-> (noisy float32 points, the clean points, their analytic normals): synth.surface_cloud displaced along its
    analytic normals by noise * N(0, 1)."""
    from pcgol_amd import synth
    clean, nrm = synth.surface_cloud(n, width, seed)
    z = np.random.default_rng(noise_seed).standard_normal(n)
    noisy = clean.astype(np.float64) + noise * z[:, None] * nrm.astype(np.float64)
    return np.ascontiguousarray(noisy, dtype=np.float32), clean, nrm


def surface_height(x, y):
    """synth.surface_cloud's h(x, y) in float64."""
    return 0.5 * np.sin(0.7 * x) * np.cos(0.5 * y) + 0.3 * np.sin(1.3 * y)


def surface_distance(p):
    """Distance of every point to the surface z = h(x, y), by Newton steps on the foot point (float64)."""
    p = np.asarray(p, np.float64)
    x, y = p[:, 0].copy(), p[:, 1].copy()
    eps = 1e-6
    for _ in range(30):
        def grad(x, y):
            dz = surface_height(x, y) - p[:, 2]
            hx = (surface_height(x + eps, y) - surface_height(x - eps, y)) / (2 * eps)
            hy = (surface_height(x, y + eps) - surface_height(x, y - eps)) / (2 * eps)
            return (x - p[:, 0]) + dz * hx, (y - p[:, 1]) + dz * hy
        gx, gy = grad(x, y)
        x, y = x - 0.5 * gx, y - 0.5 * gy  # (a damped gradient step: the surface's curvature is below 1)
    return np.sqrt((x - p[:, 0]) ** 2 + (y - p[:, 1]) ** 2 + (surface_height(x, y) - p[:, 2]) ** 2)


def interior(p, width=2.0, margin=0.15):
    """The points at least `margin` inside the surface's footprint [0, width)^2: their neighbourhoods are whole."""
    p = np.asarray(p)
    return (p[:, 0] > margin) & (p[:, 0] < width - margin) & (p[:, 1] > margin) & (p[:, 1] < width - margin)


def rms_ratio(before, after, width=2.0, margin=0.15):
    """RMS distance to the true surface over the interior points, before / after smoothing."""
    sel = interior(before, width, margin)
    rb = np.sqrt(np.mean(surface_distance(before[sel]) ** 2))
    ra = np.sqrt(np.mean(surface_distance(after[sel]) ** 2))
    return rb / ra, rb, ra


def surface_queries(base, n_inside=500, n_outside=50, seed=9):
    """Queries off the cloud: inside its bounding box, within 0.05 of the surface (a third of the tests' radius: every
    one has a neighbourhood to be projected onto), and outside the box (no neighbours)."""
    rng = np.random.default_rng(seed)
    lo, hi = base.min(0).astype(np.float64), base.max(0).astype(np.float64)
    xy = lo[:2] + rng.random((n_inside, 2)) * (hi[:2] - lo[:2])
    z = np.clip(surface_height(xy[:, 0], xy[:, 1]) + rng.uniform(-0.05, 0.05, n_inside), lo[2], hi[2])
    inside = np.column_stack([xy, z]).astype(np.float32)
    outside = (hi + 1.0 + rng.random((n_outside, 3))).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([inside, outside]), dtype=np.float32)
