// csrc/m3c2_terms.h on the host (tests/test_m3c2_terms_host.py): the expressions the kernels compile, over batches,
// through extern "C".
#include <stdint.h>

#include "m3c2_terms.h"

using namespace pcgx;

namespace {

// csrc/range_enum.h's ref_dist_sq, which the enumeration tests against the bound (float32, nothing fused)
float dist_sq(const float px, const float py, const float pz, const float qx, const float qy, const float qz) {
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return (dx * dx + dy * dy) + dz * dz;
}

Cyl cyl_at(const float *o, const float *d, const float rho, const float half_length, const int64_t i) {
  return cyl_make(o[3 * i], o[3 * i + 1], o[3 * i + 2], d[3 * i], d[3 * i + 1], d[3 * i + 2], rho, half_length);
}

}  // namespace

extern "C" {

// m (cylinder, point) pairs -> usable[i], member[i] (0 / 1), a[i], cc[i], and the range handed to the cover
void cyl_member_batch(const float *o, const float *d, float rho, float half_length, const float *p, int64_t m,
                      int32_t *usable, int32_t *member, double *a, double *cc, double *a_lo, double *a_hi) {
  for (int64_t i = 0; i < m; i++) {
    const Cyl c = cyl_at(o, d, rho, half_length, i);
    usable[i] = c.r.usable ? 1 : 0;
    a_lo[i] = c.r.a_lo, a_hi[i] = c.r.a_hi;
    member[i] = cyl_member(c, p[3 * i], p[3 * i + 1], p[3 * i + 2], a[i], cc[i]) ? 1 : 0;
  }
}

// The cover, as the kernel uses it, of m (cylinder, point) pairs, the points inside the box [lo, hi].  out = {members,
// members with a outside [a_lo, a_hi] or outside the clipped range, members without exactly one owning slab, members
// their owner's ball does not report, cylinders with more slabs than cyl_slab_bound allows}; max_slabs: the largest K.
void cyl_cover_check(const float *o, const float *d, float rho, float half_length, const float *lo, const float *hi,
                     float target, const float *p, int64_t m, int64_t *out, int32_t *max_slabs) {
  RayBox b;
  for (int k = 0; k < 3; k++) b.lo[k] = lo[k], b.hi[k] = hi[k];
  b.any = true;
  for (int k = 0; k < 5; k++) out[k] = 0;
  *max_slabs = 0;
  const double kb = cyl_slab_bound(half_length, target);
  for (int64_t i = 0; i < m; i++) {
    const Cyl c = cyl_at(o, d, rho, half_length, i);
    double a0, a1;
    const bool some = ray_clip(c.r, b, rho, a0, a1);
    const int32_t K = some ? ray_slabs(c.r, a0, a1, target) : 0;
    if (K > *max_slabs) *max_slabs = K;
    if (!((double)K <= kb)) out[4]++;
    const float bound = some ? ray_bound(c.r, b, rho, a0, a1, K) : 0.0f;
    double a, cc;
    if (!cyl_member(c, p[3 * i], p[3 * i + 1], p[3 * i + 2], a, cc)) continue;
    out[0]++;
    if (!some || !(c.r.a_lo <= a && a <= c.r.a_hi) || !(a0 <= a && a <= a1)) {
      out[1]++;
      continue;
    }
    int32_t owners = 0, owner = -1;
    for (int32_t k = 0; k < K; k++)
      if (ray_in_slab(a, a0, a1, k, K)) owners++, owner = k;
    if (owners != 1) {
      out[2]++;
      continue;
    }
    float cx, cy, cz;
    ray_centre(c.r, b, a0, a1, owner, K, cx, cy, cz);
    if (!(dist_sq(p[3 * i], p[3 * i + 1], p[3 * i + 2], cx, cy, cz) < bound)) out[3]++;
  }
}

void m3c2_finish_batch(const float *axes, const int32_t *n1, const double *s1, const int32_t *n2, const double *s2,
                       int64_t m, double registration_error, int32_t min_count, double *distance, double *lod,
                       uint8_t *significant) {
  for (int64_t i = 0; i < m; i++) {
    const M3C2Value v = m3c2_finish(axes[3 * i], axes[3 * i + 1], axes[3 * i + 2], n1[i], s1[2 * i], s1[2 * i + 1], n2[i],
                                    s2[2 * i], s2[2 * i + 1], registration_error, min_count);
    distance[i] = v.distance, lod[i] = v.lod, significant[i] = v.significant;
  }
}
}
