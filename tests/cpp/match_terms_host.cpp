// csrc/fpfh_match_terms.h on the host (tests/test_match_terms_host.py): the expressions the kernels compile, over
// batches, through extern "C".
#include <stdint.h>

#include "fpfh_match_terms.h"

using namespace pcgx;

extern "C" {

int32_t match_len() { return kMatchLen; }

// m pairs of rows -> D[i]
void match_dist_batch(const float *a, const float *b, int64_t m, float *D) {
  for (int64_t i = 0; i < m; i++) D[i] = fpfh_row_dist_sq(a + kMatchLen * i, b + kMatchLen * i);
}

// m rows -> usable[i] (0 / 1)
void match_usable_batch(const float *a, int64_t m, int32_t *usable) {
  for (int64_t i = 0; i < m; i++) usable[i] = fpfh_row_usable(a + kMatchLen * i) ? 1 : 0;
}
}
