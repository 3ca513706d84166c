// csrc/group_terms.h on the host (tests/test_group_terms_host.py): the expressions the kernels compile, over batches,
// through extern "C".
#include <stdint.h>

#include "group_terms.h"

using namespace pcgx;

extern "C" {

// m values -> their keys and the values the keys decode to
void group_keys_f32(const float *v, int64_t m, uint32_t *key, float *back) {
  for (int64_t k = 0; k < m; k++) {
    key[k] = group_key_f32(v[k]);
    back[k] = group_unkey_f32(key[k]);
  }
}
void group_keys_f64(const double *v, int64_t m, uint64_t *key, double *back) {
  for (int64_t k = 0; k < m; k++) {
    key[k] = group_key_f64(v[k]);
    back[k] = group_unkey_f64(key[k]);
  }
}

// m slots (id, xyz) of a tree of n points -> live[k] (0 / 1)
void group_live_batch(const int64_t *id, const float *xyz, int64_t n, int64_t m, int32_t *live) {
  for (int64_t k = 0; k < m; k++)
    live[k] = group_id_ok(id[k], n) && group_point_ok(xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]) ? 1 : 0;
}

// m groups: sums[10 k ..] = (sx, sy, sz, sxx, sxy, sxz, syy, syz, szz, n) about pivot[3 k ..] -> centroid, cov
void group_finish_batch(const double *sums, const double *pivot, int64_t m, double *centroid, double *cov) {
  for (int64_t k = 0; k < m; k++) {
    const double *s = sums + 10 * k;
    GroupSums a;
    a.sx = s[0]; a.sy = s[1]; a.sz = s[2];
    a.sxx = s[3]; a.sxy = s[4]; a.sxz = s[5]; a.syy = s[6]; a.syz = s[7]; a.szz = s[8];
    a.n = (int64_t)s[9];
    double c[3], q[6];
    group_finish(a, pivot[3 * k], pivot[3 * k + 1], pivot[3 * k + 2], c, q);
    for (int j = 0; j < 3; j++) centroid[3 * k + j] = c[j];
    for (int j = 0; j < 6; j++) cov[6 * k + j] = q[j];
  }
}

// m covariances -> eig[3 k ..], axes[9 k ..]
void group_frame_batch(const double *cov, int64_t m, double *eig, double *axes) {
  for (int64_t k = 0; k < m; k++) {
    double q[6], e[3], a[9];
    for (int j = 0; j < 6; j++) q[j] = cov[6 * k + j];
    group_frame(q, e, a);
    for (int j = 0; j < 3; j++) eig[3 * k + j] = e[j];
    for (int j = 0; j < 9; j++) axes[9 * k + j] = a[j];
  }
}

// m vectors, turned in place by the sign rule
void group_sign_batch(double *v, int64_t m) {
  for (int64_t k = 0; k < m; k++) group_sign(v[3 * k], v[3 * k + 1], v[3 * k + 2]);
}

// The whole call on the host, a group after the other, members in list order: m groups back to back, group k is
// points[offs[k] .. offs[k + 1]) (xyz float32, live members only).  What the kernels compute up to the order of the sums.
void group_stats_host(const float *points, const int64_t *offs, int64_t m, int64_t *count, float *aabb, double *centroid,
                      double *cov, double *eig, double *axes, double *obb) {
  for (int64_t k = 0; k < m; k++) {
    const int64_t b = offs[k], e = offs[k + 1];
    count[k] = e - b;
    for (int j = 0; j < 6; j++) aabb[6 * k + j] = 0.0f;
    for (int j = 0; j < 3; j++) centroid[3 * k + j] = eig[3 * k + j] = 0.0;
    for (int j = 0; j < 6; j++) cov[6 * k + j] = obb[6 * k + j] = 0.0;
    for (int j = 0; j < 9; j++) axes[9 * k + j] = 0.0;
    if (e == b) continue;
    uint32_t lo[3] = {kGroupKeyMin32, kGroupKeyMin32, kGroupKeyMin32}, hi[3] = {kGroupKeyMax32, kGroupKeyMax32, kGroupKeyMax32};
    for (int64_t i = b; i < e; i++)
      for (int j = 0; j < 3; j++) {
        const uint32_t key = group_key_f32(points[3 * i + j]);
        lo[j] = key < lo[j] ? key : lo[j];
        hi[j] = key > hi[j] ? key : hi[j];
      }
    double pv[3];
    for (int j = 0; j < 3; j++) {
      aabb[6 * k + j] = group_unkey_f32(lo[j]);
      aabb[6 * k + 3 + j] = group_unkey_f32(hi[j]);
      pv[j] = group_pivot(aabb[6 * k + j], aabb[6 * k + 3 + j]);
    }
    GroupSums a;
    a.clear();
    for (int64_t i = b; i < e; i++)
      a.add((double)points[3 * i] - pv[0], (double)points[3 * i + 1] - pv[1], (double)points[3 * i + 2] - pv[2]);
    double c[3], q[6], ev[3], ax[9];
    group_finish(a, pv[0], pv[1], pv[2], c, q);
    group_frame(q, ev, ax);
    uint64_t elo[3] = {kGroupKeyMin64, kGroupKeyMin64, kGroupKeyMin64}, ehi[3] = {kGroupKeyMax64, kGroupKeyMax64, kGroupKeyMax64};
    for (int64_t i = b; i < e; i++)
      for (int j = 0; j < 3; j++) {
        const uint64_t key = group_key_f64(group_extent(points[3 * i], points[3 * i + 1], points[3 * i + 2], c, ax[3 * j],
                                                        ax[3 * j + 1], ax[3 * j + 2]));
        elo[j] = key < elo[j] ? key : elo[j];
        ehi[j] = key > ehi[j] ? key : ehi[j];
      }
    const double l3[3] = {group_unkey_f64(elo[0]), group_unkey_f64(elo[1]), group_unkey_f64(elo[2])};
    const double h3[3] = {group_unkey_f64(ehi[0]), group_unkey_f64(ehi[1]), group_unkey_f64(ehi[2])};
    double box[6];
    group_obb(c, ax, l3, h3, box);
    for (int j = 0; j < 3; j++) centroid[3 * k + j] = c[j];
    for (int j = 0; j < 6; j++) cov[6 * k + j] = q[j];
    for (int j = 0; j < 3; j++) eig[3 * k + j] = ev[j];
    for (int j = 0; j < 9; j++) axes[9 * k + j] = ax[j];
    for (int j = 0; j < 6; j++) obb[6 * k + j] = box[j];
  }
}

}  // extern "C"
