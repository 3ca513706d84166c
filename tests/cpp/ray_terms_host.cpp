// csrc/ray_terms.h on the host (tests/test_ray_terms_host.py): the expressions the kernel compiles, over batches,
// through extern "C".
#include <stdint.h>

#include "ray_terms.h"

using namespace pcgx;

namespace {

// csrc/range_enum.h's ref_dist_sq, which the enumeration tests against the bound (float32, nothing fused)
float dist_sq(const float px, const float py, const float pz, const float qx, const float qy, const float qz) {
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return (dx * dx + dy * dy) + dz * dz;
}

Ray ray_at(const float *o, const float *d, const float *s_min, const float *s_max, const float rho, const int64_t i) {
  return ray_make(o[3 * i], o[3 * i + 1], o[3 * i + 2], d[3 * i], d[3 * i + 1], d[3 * i + 2], s_min[i], s_max[i], rho);
}

RayBox box_of(const float *lo, const float *hi, const int32_t any) {
  RayBox b;
  for (int k = 0; k < 3; k++) b.lo[k] = lo[k], b.hi[k] = hi[k];
  b.any = any != 0;
  return b;
}

}  // namespace

extern "C" {

void ray_constants(int32_t *cap) { *cap = kRaySlabCap; }

// m (ray, point) pairs -> usable[i], member[i] (0 / 1), a[i], cc[i]
void ray_member_batch(const float *o, const float *d, const float *s_min, const float *s_max, float rho, const float *p,
                      int64_t m, int32_t *usable, int32_t *member, double *a, double *cc) {
  for (int64_t i = 0; i < m; i++) {
    const Ray r = ray_at(o, d, s_min, s_max, rho, i);
    usable[i] = r.usable ? 1 : 0;
    member[i] = ray_member(r, p[3 * i], p[3 * i + 1], p[3 * i + 2], a[i], cc[i]) ? 1 : 0;
  }
}

void ray_beats_batch(const double *a, const int32_t *id, const double *b, const int32_t *jd, int64_t m, int32_t *out) {
  for (int64_t i = 0; i < m; i++) out[i] = ray_beats(a[i], id[i], b[i], jd[i]) ? 1 : 0;
}

void ray_clip_batch(const float *o, const float *d, const float *s_min, const float *s_max, float rho, const float *lo,
                    const float *hi, int32_t any, int64_t m, int32_t *ok, double *a0, double *a1) {
  const RayBox b = box_of(lo, hi, any);
  for (int64_t i = 0; i < m; i++) ok[i] = ray_clip(ray_at(o, d, s_min, s_max, rho, i), b, rho, a0[i], a1[i]) ? 1 : 0;
}

// The cover, as the kernel uses it, of m rays over n points inside the box [lo, hi].  slabs[i] = K of ray i (0: clipped
// away).  out = {members, members outside the clipped range, members without exactly one owning slab, members their
// owner's ball does not report, rays whose borders are not b_0 = a0 <= b_1 <= ... <= b_K = a1}.
void ray_cover_check(const float *o, const float *d, const float *s_min, const float *s_max, float rho, const float *lo,
                     const float *hi, float target, const float *p, int64_t n, int64_t m, int32_t *slabs, int64_t *out) {
  const RayBox b = box_of(lo, hi, 1);
  for (int k = 0; k < 5; k++) out[k] = 0;
  for (int64_t i = 0; i < m; i++) {
    const Ray r = ray_at(o, d, s_min, s_max, rho, i);
    double a0, a1;
    const bool some = ray_clip(r, b, rho, a0, a1);
    const int32_t K = some ? ray_slabs(r, a0, a1, target) : 0;
    slabs[i] = K;
    if (some) {
      bool good = ray_border(a0, a1, 0, K) == a0 && ray_border(a0, a1, K, K) == a1;
      for (int32_t k = 0; k < K; k++) good = good && ray_border(a0, a1, k, K) <= ray_border(a0, a1, k + 1, K);
      if (!good) out[4]++;
    }
    const float bound = some ? ray_bound(r, b, rho, a0, a1, K) : 0.0f;
    for (int64_t j = 0; j < n; j++) {
      double a, cc;
      if (!ray_member(r, p[3 * j], p[3 * j + 1], p[3 * j + 2], a, cc)) continue;
      out[0]++;
      if (!some || !(a0 <= a && a <= a1)) {
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
      ray_centre(r, b, a0, a1, owner, K, cx, cy, cz);
      if (!(dist_sq(p[3 * j], p[3 * j + 1], p[3 * j + 2], cx, cy, cz) < bound)) out[3]++;
    }
  }
}
}
