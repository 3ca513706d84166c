// csrc/gicp_terms.h on the host (tests/test_gicp_terms_host.py): the expression the kernel compiles, over batches,
// through extern "C".
#include <stdint.h>

#include "gicp_terms.h"

using namespace pcgx;

extern "C" {

int32_t gicp_chain() { return kGicpChain; }

// m pairs: p, b xyz float32; cb, ct 6 float32 each; trans16 one column-major pose -> used[i], and for used pairs
// terms[30 i ..] = {e, g[6], H[21], 1, 1}.  The rows of dropped pairs are not touched.
void gicp_terms_batch(const float *p, const float *b, const float *cb, const float *ct, const float *trans16, int64_t m,
                      int32_t *used, double *terms) {
  for (int64_t i = 0; i < m; i++) {
    double e, g[6], H[21];
    used[i] = gicp_terms(p[3 * i], p[3 * i + 1], p[3 * i + 2], b[3 * i], b[3 * i + 1], b[3 * i + 2], cb + 6 * i, ct + 6 * i,
                         trans16, e, g, H)
                  ? 1
                  : 0;
    if (!used[i]) continue;
    double *t = terms + 30 * i;
    t[0] = e;
    for (int k = 0; k < 6; k++) t[1 + k] = g[k];
    for (int k = 0; k < 21; k++) t[7 + k] = H[k];
    t[28] = t[29] = 1.0;
  }
}
}
