// csrc/mls_terms.h on the host (tests/test_mls_terms_host.py): the expressions the kernel compiles -- the frame, the
// normal equations' sums, the 6 x 6 Cholesky and the finish -- over batches of neighbourhoods, through extern "C".
#include <stdint.h>

#include "mls_terms.h"

using namespace pcgx;

extern "C" {

int32_t mls_basis() { return kMlsBasis; }
int32_t mls_sums() { return kMlsTri + kMlsBasis + 1; }
double mls_pivot_min() { return kMlsPivotMin; }

// m neighbourhoods: query i (q[3 i ..]) has the neighbours nb[3 k ..], offs[i] <= k < offs[i + 1], in that order.
// parts >= 1: the neighbours are dealt out to `parts` accumulators in turn, which are then merged (what the wave does
// with a fat row).  Out: points, normals [3 m], kinds, counts [m], pivot, c0 [m] (MlsResult).
void mls_terms_batch(const float *nb, const int64_t *offs, const float *q, int64_t m, float radius, float sigma,
                     int32_t order, int32_t min_nb, const float *vp, int32_t parts, float *points, float *normals,
                     int32_t *kinds, int32_t *counts, double *pivot, double *c0) {
  if (min_nb < 3) min_nb = 3;
  for (int64_t i = 0; i < m; i++) {
    const float qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
    NormAcc acc;
    acc.clear();
    for (int32_t part = 0; part < parts; part++) {
      NormAcc one;
      one.clear();
      for (int64_t k = offs[i] + part; k < offs[i + 1]; k += parts) one.add(nb[3 * k], nb[3 * k + 1], nb[3 * k + 2], qx, qy, qz);
      acc.merge(one);
    }
    MlsFrame F{};
    const bool framed = mls_frame(acc, min_nb, radius, sigma, F);
    const bool poly = order == 2 && framed && acc.n >= kMlsBasis;
    MlsAcc eq;
    eq.clear();
    if (poly) {
      for (int32_t part = 0; part < parts; part++) {
        MlsAcc one;
        one.clear();
        for (int64_t k = offs[i] + part; k < offs[i + 1]; k += parts)
          one.add(nb[3 * k], nb[3 * k + 1], nb[3 * k + 2], qx, qy, qz, F);
        eq.merge(one);
      }
    }
    const MlsResult R = mls_finish(framed, F, poly, eq, radius, qx, qy, qz, vp[0], vp[1], vp[2]);
    points[3 * i] = R.px; points[3 * i + 1] = R.py; points[3 * i + 2] = R.pz;
    normals[3 * i] = R.nx; normals[3 * i + 1] = R.ny; normals[3 * i + 2] = R.nz;
    kinds[i] = R.kind;
    counts[i] = acc.n;
    pivot[i] = R.pivot_ratio;
    c0[i] = R.c0;
  }
}
}
