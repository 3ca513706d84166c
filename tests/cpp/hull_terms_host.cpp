// csrc/hull_terms.h on the host (tests/test_hull_terms_host.py): the expressions the kernels compile, over batches,
// through extern "C".  PCGX_HULL_HOST_COUNT: the header counts the calls its exact branch answered.
#include <stdint.h>

#define PCGX_HULL_HOST_COUNT 1
#include "hull_terms.h"

using namespace pcgx;

extern "C" {

// m triples a, b, c (xy float32 each) -> sign[k] = hull_orient, exact[k] = 1 where the exact branch answered, and
// only[k] = hull_orient_exact's own answer
void hull_orient_batch(const float *a, const float *b, const float *c, int64_t m, int32_t *sign, int32_t *exact, int32_t *only) {
  for (int64_t k = 0; k < m; k++) {
    const long long before = g_hull_orient_fallbacks;
    sign[k] = hull_orient(a[2 * k], a[2 * k + 1], b[2 * k], b[2 * k + 1], c[2 * k], c[2 * k + 1]);
    exact[k] = g_hull_orient_fallbacks != before ? 1 : 0;
    only[k] = hull_orient_exact(a[2 * k], a[2 * k + 1], b[2 * k], b[2 * k + 1], c[2 * k], c[2 * k + 1]);
  }
}

// m places -> their keys and the coordinates the keys decode to
void hull_keys(const float *xy, int64_t m, uint64_t *key, float *back) {
  for (int64_t k = 0; k < m; k++) {
    key[k] = hull_key(xy[2 * k], xy[2 * k + 1]);
    back[2 * k] = hull_key_x(key[k]);
    back[2 * k + 1] = hull_key_y(key[k]);
  }
}

// m pairs of places -> same[k] (0 / 1)
void hull_same_place_batch(const float *a, const float *b, int64_t m, int32_t *same) {
  for (int64_t k = 0; k < m; k++) same[k] = hull_same_place(a[2 * k], a[2 * k + 1], b[2 * k], b[2 * k + 1]) ? 1 : 0;
}

// The finish of one group on the host as gh_rect_kernel has it: h vertices v (xy float32, counter-clockwise from the
// least place) -> area, rect[6]
void hull_finish_host(const float *v, int64_t h, double *area, double *rect) {
  double a = 0.0;
  if (h >= 3) {
    for (int64_t k = 1; k + 1 < h; k++) a += hull_shoelace(v[0], v[1], v[2 * k], v[2 * k + 1], v[2 * k + 2], v[2 * k + 3]);
    a *= 0.5;
  }
  *area = a;
  double out[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (h == 1) {
    out[0] = (double)v[0];
    out[1] = (double)v[1];
    out[2] = 1.0;
  } else if (h >= 2) {
    const int64_t edges = h == 2 ? 1 : h;
    double best = 0.0;
    int64_t best_k = -1;
    for (int64_t k = 0; k < edges; k++) {
      const int64_t k1 = k + 1 < h ? k + 1 : 0;
      HullExtents E;
      E.start(v[2 * k], v[2 * k + 1], v[2 * k1], v[2 * k1 + 1]);
      for (int64_t j = 0; j < h; j++) E.add(v[2 * j], v[2 * j + 1]);
      if (best_k < 0 || E.area() < best) {
        best = E.area();
        best_k = k;
      }
    }
    const int64_t k = best_k, k1 = k + 1 < h ? k + 1 : 0;
    HullExtents E;
    E.start(v[2 * k], v[2 * k + 1], v[2 * k1], v[2 * k1 + 1]);
    for (int64_t j = 0; j < h; j++) E.add(v[2 * j], v[2 * j + 1]);
    if (h == 2) E.lo_n = E.hi_n = 0.0;
    E.rect(out);
  }
  for (int j = 0; j < 6; j++) rect[j] = out[j];
}

}  // extern "C"
