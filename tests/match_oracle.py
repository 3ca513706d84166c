"""NumPy restatement of the FPFH matching contract (include/pcgx.h, "FPFH matching"), written apart from the kernels
(pcgol_amd/csrc/fpfh_match.hip, fpfh_match_terms.h):

  usable row    all 33 values finite and one of them not zero (-0.0 is zero);
  distance      acc = 0; for k = 0 .. 32: d = a[k] - b[k]; acc = acc + d * d -- every operation rounded to float32 (NumPy
                float32 arrays never fuse and never widen), vectorised over the na x nb matrix;
  match         over the usable rows j of B with finite D(i, j): the smallest (D, j) by a STABLE argsort of D (equal D
                keep ascending j), its D, the runner-up's D; {-1, inf, inf} with none or for an unusable query;
  corresp.      id >= 0, D1 <= float32(max_ratio_sq) * D2 in float32, and, if mutual, match(B, A)[id[i]] == i.

Other evaluations of the same sum (fused, widened, reversed) are here too: tests/test_match_oracle.py shows that on the
GPU tests' scene they give OTHER bits, which is what makes a bit comparison catch such a kernel."""
import numpy as np

f32, f64 = np.float32, np.float64
LEN = 33
INF = f32(np.inf)


def usable(rows):
    rows = np.asarray(rows, f32).reshape(-1, LEN)
    return np.isfinite(rows).all(axis=1) & (rows != 0).any(axis=1)


def dist_matrix(A, B):
    """D[i, j], float32, the contract's loop"""
    A = np.asarray(A, f32).reshape(-1, LEN)
    B = np.asarray(B, f32).reshape(-1, LEN)
    acc = np.zeros((len(A), len(B)), f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(LEN):
            d = A[:, k, None] - B[None, :, k]
            assert d.dtype == f32
            acc = acc + d * d
    return acc


def dist_matrix_fma(A, B):
    """the same sum as an fmaf chain: acc = fma(d, d, acc) -- d * d exact in float64 (24 + 24 bits), the sum with the
    float32 acc rounded once (float64 holds it to 53 bits: double rounding would need a tie at bit 29 beyond)"""
    A = np.asarray(A, f32).reshape(-1, LEN)
    B = np.asarray(B, f32).reshape(-1, LEN)
    acc = np.zeros((len(A), len(B)), f32)
    for k in range(LEN):
        d = (A[:, k, None] - B[None, :, k]).astype(f64)
        acc = (d * d + acc.astype(f64)).astype(f32)
    return acc


def dist_matrix_f64(A, B):
    """float64 throughout, rounded to float32 once"""
    A = np.asarray(A, f32).reshape(-1, LEN).astype(f64)
    B = np.asarray(B, f32).reshape(-1, LEN).astype(f64)
    acc = np.zeros((len(A), len(B)), f64)
    for k in range(LEN):
        d = A[:, k, None] - B[None, :, k]
        acc = acc + d * d
    return acc.astype(f32)


def dist_matrix_reversed(A, B):
    """the contract's float32 loop with k running downward"""
    A = np.asarray(A, f32).reshape(-1, LEN)
    B = np.asarray(B, f32).reshape(-1, LEN)
    return dist_matrix(A[:, ::-1], B[:, ::-1])


def match_from(D, ua, ub):
    """the match from a distance matrix and the two usable masks -> ids int64, d1, d2 float32"""
    na, nb = D.shape
    ids = np.full(na, -1, np.int64)
    d1 = np.full(na, INF, f32)
    d2 = np.full(na, INF, f32)
    if na == 0 or nb == 0:
        return ids, d1, d2
    E = np.where(ub[None, :] & np.isfinite(D), D, INF).astype(f32)  # who is no candidate sorts last
    order = np.argsort(E, axis=1, kind="stable")[:, :2]
    rows = np.arange(na)
    b1 = E[rows, order[:, 0]]
    got = ua & np.isfinite(b1)
    ids[got] = order[got, 0]
    d1[got] = b1[got]
    if nb > 1:
        d2[got] = E[rows, order[:, 1]][got]
    return ids, d1, d2


def match(A, B, dist=dist_matrix):
    A = np.asarray(A, f32).reshape(-1, LEN)
    B = np.asarray(B, f32).reshape(-1, LEN)
    return match_from(dist(A, B), usable(A), usable(B))


def correspondences_from_matches(ids, d1, d2, back, max_ratio_sq=1.0, mutual=True):
    """the correspondences from the match of A in B (ids, d1, d2) and the ids of the match of B in A (back; not read
    unless mutual) -> (m, 2) int64"""
    with np.errstate(invalid="ignore"):
        keep = (ids >= 0) & (d1 <= f32(max_ratio_sq) * d2)
    if mutual and len(back) > 0:
        keep &= back[np.where(ids >= 0, ids, 0)] == np.arange(len(ids))
    src = np.nonzero(keep)[0]
    return np.stack([src, ids[src]], axis=1).astype(np.int64)


def correspondences_from(D, ua, ub, max_ratio_sq=1.0, mutual=True):
    """the correspondences from a distance matrix and the two usable masks -> (m, 2) int64"""
    ids, d1, d2 = match_from(D, ua, ub)
    # (the match of B in A from the transposed matrix: D is bit-symmetric, tests/test_match_oracle.py)
    back = match_from(np.ascontiguousarray(D.T), ub, ua)[0] if mutual else None
    return correspondences_from_matches(ids, d1, d2, back, max_ratio_sq, mutual)


def correspondences(A, B, max_ratio_sq=1.0, mutual=True):
    """-> (m, 2) int64, ascending in the first column"""
    A = np.asarray(A, f32).reshape(-1, LEN)
    B = np.asarray(B, f32).reshape(-1, LEN)
    return correspondences_from(dist_matrix(A, B), usable(A), usable(B), max_ratio_sq, mutual)


def scene_r(na=3000, nb=2999, seed=7):
    """Scene R: rows that look like FPFH rows -- per feature a multinomial count c of 40 over 11 bins (the SPFH term,
    100 c / 40) plus random weights scaled to 100 (the neighbours' term) -- so that distances are sums of 33 squares
    of very different sizes.  A is drawn first (its counts, then its weights), then B.
    -> A (na, 33), B (nb, 33) float32"""
    rng = np.random.default_rng(seed)

    def rows(n):
        c = rng.multinomial(40, np.full(11, 1.0 / 11.0), size=(n, 3)).astype(f64)
        w = rng.uniform(0.0, 1.0, (n, 3, 11)) * 40.0
        F = 100.0 * c / 40.0 + 100.0 * w / w.sum(axis=2, keepdims=True)
        return np.ascontiguousarray(F.astype(f32).reshape(n, LEN))

    A = rows(na)
    return A, rows(nb)
