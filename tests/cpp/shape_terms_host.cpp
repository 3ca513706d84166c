// csrc/shape_terms.h on the host (tests/test_shape_terms_host.py): the expressions the kernels of shapes.hip compile, as
// a shared library of batch entry points over the shim tests/cpp/host_shim.
#include <stdint.h>

#include "shape_terms.h"

using namespace pcgx;

extern "C" {

// pairs[12 k ..]: p0, n0, p1, n1; has[k]: the seed has a partner; axis: 3 floats or NULL -> status[k], recs[8 k ..]
void shape_hypothesis_batch(int32_t kind, const float *pairs, const int32_t *has, int64_t m, const float *axis,
                            float min_axis_cos, float r_min, float r_max, int32_t *status, float *recs) {
  const PlaneAxis A = plane_axis(axis, min_axis_cos);
  for (int64_t k = 0; k < m; k++)
    status[k] = shape_hypothesis(kind, has[k] != 0, pairs + 12 * k, pairs + 12 * k + 3, pairs + 12 * k + 6,
                                 pairs + 12 * k + 9, A, r_min, r_max, recs + 8 * k);
}

// one record against m points and their normals -> in[k]
void shape_inlier_batch(int32_t kind, const float *rec8, const float *pts, const float *nrm, int64_t m, float max_dist,
                        float min_normal_cos, int32_t *in) {
  float lo2, hi2;
  shape_band(rec8[3], max_dist, &lo2, &hi2);
  const float c2 = min_normal_cos * min_normal_cos;
  for (int64_t k = 0; k < m; k++)
    in[k] = shape_inlier_any(kind, min_normal_cos != 0.0f, rec8, lo2, hi2, c2, pts[3 * k], pts[3 * k + 1], pts[3 * k + 2],
                             nrm[3 * k], nrm[3 * k + 1], nrm[3 * k + 2])
                ? 1 : 0;
}

void shape_band_batch(const float *r, int64_t m, float max_dist, float *lo2, float *hi2) {
  for (int64_t k = 0; k < m; k++) shape_band(r[k], max_dist, lo2 + k, hi2 + k);
}

void shape_mix_batch(const uint32_t *u1, const uint32_t *id, int64_t m, uint32_t *x, uint64_t *key) {
  for (int64_t k = 0; k < m; k++) {
    x[k] = shape_mix(u1[k], id[k]);
    key[k] = shape_partner_key(u1[k], id[k]);
  }
}

// the terms of one record's refit: coords[3 k ..] and terms[13 k ..] of the m points
void shape_refit_terms_batch(int32_t kind, const float *rec8, const float *pts, int64_t m, double *coords, double *terms) {
  for (int64_t k = 0; k < m; k++) {
    shape_refit_coords(kind, rec8, pts + 3 * k, coords + 3 * k);
    shape_refit_terms(coords + 3 * k, terms + 13 * k);
  }
}

// sums[13 k ..] over n[k] points about recs[8 k ..] -> ok[k], out[8 k ..]
void shape_refit_batch(int32_t kind, const float *recs, const double *n, const double *sums, int64_t m, float r_min,
                       float r_max, int32_t *ok, float *out) {
  for (int64_t k = 0; k < m; k++)
    ok[k] = shape_refit(kind, recs + 8 * k, n[k], sums + 13 * k, r_min, r_max, out + 8 * k) ? 1 : 0;
}

void shape_codes(int32_t *out8) {
  out8[0] = kShapeNotRun;
  out8[1] = kShapeOk;
  out8[2] = kShapeNoPartner;
  out8[3] = kShapeDegenerate;
  out8[4] = kShapeAxis;
  out8[5] = kShapeRadius;
  out8[6] = kShapeSphere;
  out8[7] = kShapeCylinder;
}
}
