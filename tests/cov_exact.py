"""Exact restatement of the neighbourhood covariance (include/pcgx.h, pcgx_kdtree_covariances / pcgx_kdtree_normals;
csrc/cov3.h), for the lists where tests/cov_oracle.py's float64 formula cancels.

The inputs are float32, so every d = p - q and every moment is a rational with a power-of-two denominator.  The list's
coordinates are brought to integers by one common power of two, the moments are summed in Python integers and divided
as fractions.Fraction; every result is rounded to float64 once, at the end.  For one query with neighbours p_j taken
w_j times (n = sum w_j):
  C   = sum w d d^T / n - m m^T, m = sum w d / n          (xx, xy, xz, yy, yz, zz)
  tr  = trace(C);  S = sum w |d|^2 / n                    (the uncentred second moment about the query)
  lam, vec = numpy.linalg.eigh(C / tr): the unit-trace eigenvalues, ascending, and eigenvectors in columns
  B   = (2 n + 4) 2^-53 S: the forward error bound of sum d d^T / n - m m^T evaluated in float64 in any summation order
        (n products and n additions per sum, the mean's product, the final subtraction; |m|^2 <= S).
Degenerate (n < 3, or tr == 0 exactly: every neighbour at one place): C = 0, lam NaN, vec 0."""
from fractions import Fraction

import numpy as np

UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
U53 = 2.0 ** -53


def _integers(vals):
    """float32 values -> (Python ints, e) with value = int * 2^e exactly"""
    v = np.asarray(vals, np.float32).astype(np.float64).ravel()
    nz = v[v != 0.0]
    if len(nz) == 0:
        return [0] * len(v), 0
    e = int(np.frexp(nz)[1].min()) - 24  # a float32 x is a multiple of 2^(exponent(x) - 24), subnormals included
    return [int(x) for x in np.ldexp(v, -e)], e


def one(points, q, weights=None):
    """The exact moments of one list: points (n, 3) float32, q (3,) float32, weights (n,) int or None ->
    dict(n, cov6 f64 (6,), trace, S, B, degenerate)."""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    q = np.asarray(q, np.float32).reshape(3)
    w = [1] * len(P) if weights is None else [int(x) for x in weights]
    n = sum(w)
    if n == 0 or not (np.all(np.isfinite(q)) and np.all(np.isfinite(P))):
        return dict(n=n, cov6=np.zeros(6), trace=0.0, S=0.0, B=0.0, degenerate=True)
    ints, e = _integers(np.concatenate([P.ravel(), q]))
    qi = ints[-3:]
    s1 = [0, 0, 0]
    s2 = [0] * 6
    for j in range(len(P)):
        d = (ints[3 * j] - qi[0], ints[3 * j + 1] - qi[1], ints[3 * j + 2] - qi[2])
        for a in range(3):
            s1[a] += w[j] * d[a]
        for c, (a, b) in enumerate(UPPER):
            s2[c] += w[j] * d[a] * d[b]
    scale = Fraction(2) ** (2 * e)
    cov = [Fraction(n * s2[c] - s1[a] * s1[b], n * n) * scale for c, (a, b) in enumerate(UPPER)]
    tr = cov[0] + cov[3] + cov[5]
    S = float(Fraction(s2[0] + s2[3] + s2[5], n) * scale)
    degenerate = n < 3 or tr == 0
    cov6 = np.zeros(6) if degenerate else np.array([float(x) for x in cov])
    return dict(n=n, cov6=cov6, trace=0.0 if degenerate else float(tr), S=S, B=(2 * n + 4) * U53 * S,
                degenerate=degenerate)


def full(cov6):
    """(m, 6) -> (m, 3, 3) symmetric"""
    c = np.asarray(cov6, np.float64)
    M = np.empty(c.shape[:-1] + (3, 3))
    for k, (a, b) in enumerate(UPPER):
        M[..., a, b] = M[..., b, a] = c[..., k]
    return M


def from_lists(points, queries, lists, merge_above=64):
    """lists: one id array per query -> dict(n i64 (m,), cov6 f64 (m,6), trace, S, B f64 (m,), lam f64 (m,3), vec f64
    (m,3,3), degenerate bool (m,)).  A list longer than merge_above is summed with multiplicities (coincident heaps)."""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    Q = np.asarray(queries, np.float32).reshape(-1, 3)
    m = len(Q)
    out = dict(n=np.zeros(m, np.int64), cov6=np.zeros((m, 6)), trace=np.zeros(m), S=np.zeros(m), B=np.zeros(m),
               lam=np.full((m, 3), np.nan), vec=np.zeros((m, 3, 3)), degenerate=np.ones(m, bool))
    for i in range(m):
        pj = P[np.asarray(lists[i], np.int64)]
        w = None
        if len(pj) > merge_above:
            pj, w = np.unique(pj, axis=0, return_counts=True)
        o = one(pj, Q[i], w)
        for key in ("n", "cov6", "trace", "S", "B", "degenerate"):
            out[key][i] = o[key]
    ok = ~out["degenerate"]
    if ok.any():
        lam, vec = np.linalg.eigh(full(out["cov6"][ok]) / out["trace"][ok][:, None, None])
        out["lam"][ok] = lam
        out["vec"][ok] = vec
    return out


def knn_lists(ids, counts):
    """knn_oracle.knearest's (ids, counts) -> one id array per query"""
    return [np.asarray(ids[i, :counts[i]], np.int64) for i in range(len(counts))]


def csr_lists(offs, ids):
    """(offsets, ids) as normals_oracle.range_lists returns them -> one id array per query"""
    return [np.asarray(ids[offs[i]:offs[i + 1]], np.int64) for i in range(len(offs) - 1)]
