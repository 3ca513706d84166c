// csrc/ndt_terms.h on the host (tests/test_ndt_terms_host.py): the expressions the kernels compile -- the voxel finish,
// Magnusson's constants and one pair's terms -- over batches, through extern "C".
#include <stdint.h>

#include "ndt_terms.h"

using namespace pcgx;

extern "C" {

int32_t ndt_chain() { return kNdtChain; }

int32_t ndt_k2_host(float outlier_ratio, float resolution, double *k2) { return ndt_k2(outlier_ratio, resolution, k2) ? 1 : 0; }

// m voxels: voxel i has the points pts[3 k ..], offs[i] <= k < offs[i + 1], in that order, and the integer coordinates
// v[3 i ..] in the grid (origin, resolution).  parts >= 1: the points are dealt out to `parts` accumulators in turn,
// which are then merged (what the wave's lanes do).
void ndt_voxels_batch(const float *pts, const int64_t *offs, const int64_t *v, int64_t m, const float *origin,
                      float resolution, int32_t min_points, float ratio, int32_t parts, int32_t *count, int32_t *valid,
                      float *mean3, float *cov6, float *icov6) {
  for (int64_t i = 0; i < m; i++) {
    const double ox = ndt_centre(origin[0], v[3 * i], resolution), oy = ndt_centre(origin[1], v[3 * i + 1], resolution),
                 oz = ndt_centre(origin[2], v[3 * i + 2], resolution);
    NormAcc acc;
    acc.clear();
    for (int32_t part = 0; part < parts; part++) {
      NormAcc one;
      one.clear();
      for (int64_t k = offs[i] + part; k < offs[i + 1]; k += parts) ndt_acc_add(one, pts[3 * k], pts[3 * k + 1], pts[3 * k + 2], ox, oy, oz);
      acc.merge(one);
    }
    NdtVoxel out;
    valid[i] = ndt_voxel_finish(acc, ox, oy, oz, min_points, ratio, out) ? 1 : 0;
    count[i] = acc.n;
    for (int k = 0; k < 3; k++) mean3[3 * i + k] = out.mean[k];
    for (int k = 0; k < 6; k++) {
      cov6[6 * i + k] = out.cov6[k];
      icov6[6 * i + k] = out.icov6[k];
    }
  }
}

// n pairs -> terms[30 i ..] = {e, g[6], H[21], w, 1}
void ndt_pairs_batch(const float *p, const float *mean, const float *icov6, int64_t n, double k2, double *terms) {
  for (int64_t i = 0; i < n; i++) {
    double *t = terms + 30 * i;
    ndt_pair_terms(p[3 * i], p[3 * i + 1], p[3 * i + 2], mean + 3 * i, icov6 + 6 * i, 0.5 * k2, 2.0 / k2, t[0], t + 1, t + 7,
                   t[28]);
    t[29] = 1.0;
  }
}
}
