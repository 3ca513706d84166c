// csrc/thin_terms.h on the host (tests/test_thin_terms_host.py): the expressions the kernels compile, as a program of
// its own, built with -fsanitize=address,undefined.  It reads a table from stdin and prints one line per row.
//   first line: m k          m points, k pairs
//   m lines:    id score     id decimal, score as the 8 hex digits of its float32
//   k lines:    seed a b     the pair (point a, point b) under that seed
// and answers, per pair: before_hash before_score score_ok_a eligible_a(met = 1) key_a(hex) owner_beats, where
// owner_beats takes the two scores as distances; then the eight rows of thin_decide's table and the constants.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "thin_terms.h"

using namespace pcgx;

int main() {
  long long m = 0, k = 0;
  if (scanf("%lld %lld", &m, &k) != 2 || m < 0 || k < 0) return 2;
  std::vector<uint32_t> id((size_t)m);
  std::vector<float> score((size_t)m);
  for (long long r = 0; r < m; r++) {
    uint32_t bits = 0;
    if (scanf("%" SCNu32 " %" SCNx32, &id[(size_t)r], &bits) != 2) return 2;
    memcpy(&score[(size_t)r], &bits, 4);
  }
  for (long long r = 0; r < k; r++) {
    uint32_t seed = 0;
    long long a = 0, b = 0;
    if (scanf("%" SCNu32 " %lld %lld", &seed, &a, &b) != 3 || a < 0 || a >= m || b < 0 || b >= m) return 2;
    const uint32_t ia = id[(size_t)a], ib = id[(size_t)b];
    const float sa = score[(size_t)a], sb = score[(size_t)b];
    printf("%d %d %d %d %016" PRIx64 " %d\n", thin_before(false, seed, sa, ia, sb, ib) ? 1 : 0,
           thin_before(true, seed, sa, ia, sb, ib) ? 1 : 0, thin_score_ok(true, sa) ? 1 : 0,
           thin_eligible(true, true, sa) ? 1 : 0, shape_partner_key(seed, ia), thin_owner_beats(sa, ia, sb, ib) ? 1 : 0);
  }
  for (int e = 0; e < 2; e++)
    for (int kb = 0; kb < 2; kb++)
      for (int ub = 0; ub < 2; ub++) printf("decide %d %d %d %d\n", e, kb, ub, (int)thin_decide(e != 0, kb != 0, ub != 0));
  printf("states %d %d %d %d\n", (int)kThinUndecided, (int)kThinKept, (int)kThinDropped, (int)kThinIneligible);
  printf("owner %d %d\n", (int)kThinNoOwner, (int)kThinNotRun);
  printf("hash_mode %d %d %d\n", thin_score_ok(false, __builtin_nanf("")) ? 1 : 0,
         thin_eligible(true, false, __builtin_nanf("")) ? 1 : 0, thin_eligible(false, false, 1.0f) ? 1 : 0);
  return 0;
}
