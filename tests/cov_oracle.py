"""float64 NumPy restatement of k-NN covariances (include/pcgx.h, pcgx_kdtree_covariances; csrc/knearest.hip).

No reference counterpart exists: this is the contract itself.  For query q with neighbour list N(q) (the ids
tests/knn_oracle.py gives, n = |N(q)|), mode and epsilon:
  d = p - q in float64, m = sum d / n, C = sum d d^T / n - m m^T;
  degenerate (n < 3, or all of N(q) at one place): RAW 0, PLANE I, normal 0;
  RAW: C;  PLANE: I - (1 - eps) u u^T with u the unit eigenvector of C's smallest eigenvalue;
  normal: u, negated where u . (v - q) < 0.
Six values per query: xx, xy, xz, yy, yz, zz.

This is the well-conditioned restatement: it evaluates the kernel's formula in the kernel's precision, so where that
formula cancels (a query far from its neighbours compared with their spread) it is as wrong as the kernel, differently.
tests/cov_exact.py is the reference that is exact there (rational arithmetic, with a derived error bound for the
float64 formula); tests/test_gpu_cov_conditioning.py compares the kernels with it."""
import numpy as np

RAW, PLANE = 0, 1
UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def covariances(points, queries, ids, counts, mode=PLANE, eps=1e-3, viewpoint=(0.0, 0.0, 0.0)):
    """ids (m, k) / counts (m,) as knn_oracle.knearest returns them -> dict(cov6 f64 (m,6), normals f64 (m,3),
    lam f64 (m,3) ascending (NaN where degenerate), degenerate bool (m,), trace f64 (m,) of C (0 where degenerate))."""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    Q = np.asarray(queries, np.float32).reshape(-1, 3)
    ids = np.asarray(ids, np.int64)
    counts = np.asarray(counts, np.int64)
    m, k = ids.shape
    valid = np.arange(k)[None, :] < counts[:, None]
    pj = P[np.where(valid, ids, 0)]
    lo = np.where(valid[:, :, None], pj, np.inf).min(1)
    hi = np.where(valid[:, :, None], pj, -np.inf).max(1)
    degen = (counts < 3) | ~np.any(lo != hi, axis=1)
    d = np.where(valid[:, :, None], pj.astype(np.float64) - Q[:, None, :].astype(np.float64), 0.0)
    n = np.maximum(counts, 1).astype(np.float64)
    mean = d.sum(1) / n[:, None]
    C = np.einsum("mki,mkj->mij", d, d) / n[:, None, None] - mean[:, :, None] * mean[:, None, :]
    C[degen] = 0.0
    tr = np.trace(C, axis1=1, axis2=2)
    w, V = np.linalg.eigh(C)
    u = V[:, :, 0] / np.linalg.norm(V[:, :, 0], axis=1, keepdims=True)
    v = np.asarray(viewpoint, np.float32).astype(np.float64)
    u[np.sum(u * (v[None, :] - Q.astype(np.float64)), axis=1) < 0] *= -1.0
    if mode == RAW:
        out = C
    else:
        f = 1.0 - float(np.float32(eps))
        out = np.eye(3)[None, :, :] - f * u[:, :, None] * u[:, None, :]
        out[degen] = np.eye(3)
    u[degen] = 0.0
    w[degen] = np.nan
    cov6 = np.stack([out[:, i, j] for i, j in UPPER], axis=1)
    return dict(cov6=cov6, normals=u, lam=w, degenerate=degen, trace=tr)
