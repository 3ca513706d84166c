// csrc/fps_terms.h on the host (tests/test_fps_terms_host.py): the expressions the kernels compile, as a program of its
// own, built with -ffp-contract=off -fsanitize=address,undefined.  It reads from stdin
//   first line: m k            m key rows, k lemma triples
//   m lines:    d id           d as the 8 hex digits of its float32, id decimal
//   k lines:    18 hex words   lo[3] hi[3] p[3] s[3] of one triple (lo <= p <= hi is the test's business)
// and prints per key row "key(hex) id d(hex)", then per triple "lower(hex) dist(hex) ok skips_at_dist", then the
// constants.  ok = lower <= dist, the lemma.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "fps_terms.h"

using namespace pcgx;

static bool word(float *f) {
  uint32_t u = 0;
  if (scanf("%" SCNx32, &u) != 1) return false;
  *f = fps_from_bits(u);
  return true;
}

int main() {
  long long m = 0, k = 0;
  if (scanf("%lld %lld", &m, &k) != 2 || m < 0 || k < 0) return 2;
  for (long long r = 0; r < m; r++) {
    float d = 0.0f;
    uint32_t id = 0;
    if (!word(&d) || scanf("%" SCNu32, &id) != 1) return 2;
    const uint64_t key = fps_key(d, id);
    printf("%016" PRIx64 " %" PRIu32 " %08" PRIx32 "\n", key, fps_key_id(key), fps_bits(fps_key_d(key)));
  }
  for (long long r = 0; r < k; r++) {
    float v[12];
    for (int i = 0; i < 12; i++)
      if (!word(&v[i])) return 2;
    const float lower = fps_box_lower(v[9], v[10], v[11], v[0], v[1], v[2], v[3], v[4], v[5]);
    const float dist = ref_dist_sq(v[6], v[7], v[8], v[9], v[10], v[11]);
    printf("%08" PRIx32 " %08" PRIx32 " %d %d\n", fps_bits(lower), fps_bits(dist), lower <= dist ? 1 : 0,
           fps_skips(lower, dist) ? 1 : 0);
  }
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
  printf("updates %d %d %d %d\n", fps_updates(1.0f, 2.0f) ? 1 : 0, fps_updates(2.0f, 2.0f) ? 1 : 0,
         fps_updates(0.0f, inf) ? 1 : 0, fps_updates(inf, inf) ? 1 : 0);
  printf("eligible %d %d %d %d\n", fps_eligible(1.0f, -2.0f, 0.0f) ? 1 : 0, fps_eligible(nan, 0.0f, 0.0f) ? 1 : 0,
         fps_eligible(0.0f, inf, 0.0f) ? 1 : 0, fps_eligible(0.0f, 0.0f, -inf) ? 1 : 0);
  printf("skips %d %d %d %d\n", fps_skips(0.0f, 0.0f) ? 1 : 0, fps_skips(1.0f, 1.0f) ? 1 : 0, fps_skips(1.0f, 2.0f) ? 1 : 0,
         fps_skips(nan, 0.0f) ? 1 : 0);
  printf("padding %d %08" PRIx32 " %" PRIu32 "\n", (int)kFpsNoId, fps_bits(kFpsNoDist), kFpsMaxId);
  return 0;
}
