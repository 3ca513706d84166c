// csrc/ground_terms.h on the host (tests/test_ground_terms_host.py): the expressions the kernels of ground.hip compile, as
// a shared library of batch entry points over the shim tests/cpp/host_shim.
#include <math.h>
#include <stdint.h>

#include "ground_terms.h"

using namespace pcgx;

extern "C" {

// pts[3 k ..] -> cell[k] (-1: not live)
void ground_cell_batch(const float *pts, int64_t m, const float *origin, const int32_t *dims, float cell, int32_t *out) {
  const GroundGrid g = {origin[0], origin[1], cell, dims[0], dims[1]};
  for (int64_t k = 0; k < m; k++) out[k] = ground_cell(g, pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]);
}

// z[k] -> key[k], back[k] = the float the key stands for, surface[k] = what the surface output shows for the key
void ground_key_batch(const float *z, int64_t m, uint32_t *key, float *back, float *surface) {
  for (int64_t k = 0; k < m; k++) {
    key[k] = ground_key(z[k]);
    back[k] = group_unkey_f32(key[k]);
    surface[k] = ground_surface(key[k]);
  }
}

// a cell word through a pass: in[k] = what an erosion (is_max 0) or a dilation (1) reads, out[k] = what it writes for it,
// op[k] = the combine of words[k] and words[k + 1 mod m] as read
void ground_morph_batch(const uint32_t *words, int64_t m, int32_t is_max, uint32_t *in, uint32_t *out, uint32_t *op) {
  for (int64_t k = 0; k < m; k++) {
    const uint32_t a = words[k], b = words[(k + 1) % m];
    if (is_max) {
      in[k] = ground_morph_in<true>(a);
      out[k] = ground_morph_out<true>(in[k]);
      op[k] = ground_morph_op<true>(ground_morph_in<true>(a), ground_morph_in<true>(b));
    } else {
      in[k] = ground_morph_in<false>(a);
      out[k] = ground_morph_out<false>(in[k]);
      op[k] = ground_morph_op<false>(ground_morph_in<false>(a), ground_morph_in<false>(b));
    }
  }
}

// z[k] over the surface value s[k] against height[k] -> survives[k], hag[k]
void ground_test_batch(const float *z, const float *s, const float *height, int64_t m, int32_t *survives, float *hag) {
  for (int64_t k = 0; k < m; k++) {
    const uint32_t w = ground_key(s[k]);
    survives[k] = ground_survives(z[k], w, height[k]) ? 1 : 0;
    hag[k] = ground_hag(z[k], w);
  }
}

void ground_constants(uint32_t *out2) {
  out2[0] = kGroundEmpty;
  out2[1] = kGroundHagNone;
}
}
