"""float64 NumPy restatement of statistical outlier removal (include/pcgx.h, pcgx_sor_filter; csrc/sor.hip) on top of
the brute-force k-NN oracle (tests/knn_oracle.py).

  F   = the points whose x, y, z are all finite; m = |F|; ids are positions in F;
  d_i = (1/mean_k) * sum of sqrt(float64(DistSq)) over the mean_k points of F \\ {i} with the smallest (DistSq, id),
        summed in that order;
  mu  = sum d_i / m; sigma = sqrt(sum (d_i - mu)^2 / (m - 1)); T = mu + std_mul * sigma;
  keep i iff d_i <= T (negative: d_i > T); non-finite points are kept in neither mode."""
import numpy as np

import knn_oracle as KO


class NoPoint(Exception):
    pass


def mean_dists(xyz, mean_k):
    """-> (mean_dist float64 [n] by input index, NaN for non-finite points; finite mask)."""
    P = np.asarray(xyz, np.float32).reshape(-1, 3)
    fin = np.all(np.isfinite(P), axis=1)
    F = P[fin]
    m = len(F)
    if m <= mean_k:
        raise NoPoint("m = %d <= mean_k = %d" % (m, mean_k))
    ids, dsq, counts = KO.knearest(F, F, mean_k + 1, np.inf)
    # the first mean_k entries that are not the point itself (it is dropped if present, else the last entry is)
    take = (ids >= 0) & (ids != np.arange(m)[:, None])
    take &= np.cumsum(take, 1) <= mean_k
    s = np.zeros(m, np.float64)
    for c in range(ids.shape[1]):  # in ascending order, as the contract sums
        v = np.sqrt(dsq[:, c].astype(np.float64))
        s = np.where(take[:, c], s + v, s)
    d = s / mean_k
    out = np.full(len(P), np.nan)
    out[fin] = d
    return out, fin


def sor(xyz, mean_k, std_mul, negative=False):
    """-> dict(keep bool [n], mean_dist float64 [n], mu, sigma, T)."""
    md, fin = mean_dists(xyz, mean_k)
    d = md[fin]
    m = len(d)
    mu = d.sum() / m
    sigma = np.sqrt(((d - mu) ** 2).sum() / (m - 1))
    T = mu + np.float64(np.float32(std_mul)) * sigma
    with np.errstate(invalid="ignore"):
        keep = (md > T) if negative else (md <= T)
    return dict(keep=keep, mean_dist=md, mu=mu, sigma=sigma, T=T)
