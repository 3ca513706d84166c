// csrc/fpfh_terms.h on the host (tests/test_fpfh_terms_host.py): the expression the kernel compiles, over batches,
// through extern "C".
#include <stdint.h>

#include "fpfh_terms.h"

using namespace pcgx;

extern "C" {

int32_t fpfh_len() { return kFpfhLen; }

// m pairs: ps, ns, pt, nt xyz float32 -> valid[i], and for valid pairs bins[3 i ..] = {b1, b2, b3}.  The rows of
// invalid pairs are not touched.
void fpfh_terms_batch(const float *ps, const float *ns, const float *pt, const float *nt, int64_t m, int32_t *valid,
                      int32_t *bins) {
  for (int64_t i = 0; i < m; i++) {
    int b1, b2, b3;
    valid[i] = fpfh_terms(ps[3 * i], ps[3 * i + 1], ps[3 * i + 2], ns[3 * i], ns[3 * i + 1], ns[3 * i + 2], pt[3 * i],
                          pt[3 * i + 1], pt[3 * i + 2], nt[3 * i], nt[3 * i + 1], nt[3 * i + 2], b1, b2, b3)
                   ? 1
                   : 0;
    if (!valid[i]) continue;
    bins[3 * i] = b1;
    bins[3 * i + 1] = b2;
    bins[3 * i + 2] = b3;
  }
}
}
