// csrc/plane_terms.h on the host (tests/test_plane_terms_host.py): the expressions the kernels of planes.hip compile, as
// a shared library of batch entry points over the shim tests/cpp/host_shim.
#include <stdint.h>

#include "plane_terms.h"

using namespace pcgx;

extern "C" {

// tri[9 k ..]: p0, p1, p2; idx[3 k ..]: their indices; axis: 3 floats or NULL -> status[k], planes[4 k ..]
void plane_hypothesis_batch(const float *tri, const uint32_t *idx, int64_t m, const float *axis, float min_axis_cos,
                            int32_t *status, float *planes) {
  const PlaneAxis A = plane_axis(axis, min_axis_cos);
  for (int64_t k = 0; k < m; k++)
    status[k] = plane_hypothesis(idx[3 * k], idx[3 * k + 1], idx[3 * k + 2], tri + 9 * k, tri + 9 * k + 3, tri + 9 * k + 6, A,
                                 planes + 4 * k);
}

// frames[7 k ..]: centroid, axis 2, eig[0] -> ok[k], planes[4 k ..]
void plane_refit_batch(const double *frames, int64_t m, const float *axis, float min_axis_cos, int32_t *ok, float *planes) {
  const PlaneAxis A = plane_axis(axis, min_axis_cos);
  for (int64_t k = 0; k < m; k++)
    ok[k] = plane_refit(frames + 7 * k, frames + 7 * k + 3, frames[7 * k + 6], A, planes + 4 * k) ? 1 : 0;
}

// one plane against m points (and their normals, or NULL) -> in[k]
void plane_inlier_batch(const float *plane4, const float *pts, const float *nrm, int64_t m, float max_dist,
                        float min_normal_cos, int32_t *in) {
  for (int64_t k = 0; k < m; k++) {
    bool ok = plane_near(plane4, pts[3 * k], pts[3 * k + 1], pts[3 * k + 2], max_dist);
    if (nrm) ok = ok && plane_normal_agrees(plane4, nrm[3 * k], nrm[3 * k + 1], nrm[3 * k + 2], min_normal_cos);
    in[k] = ok ? 1 : 0;
  }
}

// live[k]: bit 0 the point test, bit 1 the normal test, of the three floats v[3 k ..]
void plane_live_batch(const float *v, int64_t m, int32_t *live) {
  for (int64_t k = 0; k < m; k++)
    live[k] = (plane_point_live(v[3 * k], v[3 * k + 1], v[3 * k + 2]) ? 1 : 0) |
              (plane_normal_live(v[3 * k], v[3 * k + 1], v[3 * k + 2]) ? 2 : 0);
}

void plane_sample_batch(const uint32_t *u, const uint32_t *m, int64_t k, uint32_t *out) {
  for (int64_t i = 0; i < k; i++) out[i] = pose_sample_index(u[i], m[i]);
}

void plane_status_codes(int32_t *out5) {
  out5[0] = kPlaneNotRun;
  out5[1] = kPlaneOk;
  out5[2] = kPlaneBadSample;
  out5[3] = kPlaneDegenerate;
  out5[4] = kPlaneAxis;
}
}
