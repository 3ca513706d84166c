// csrc/dbscan_terms.h on the host (tests/test_dbscan_terms_host.py): the expressions the kernels compile, over batches,
// through extern "C".
#include <stdint.h>

#include "dbscan_terms.h"

using namespace pcgx;

extern "C" {

// m pairs of candidates -> beats[k] (0 / 1): does (d, id) beat (best_d, best_id)?
void dbscan_beats_batch(const float *d, const uint32_t *id, const float *best_d, const uint32_t *best_id, int64_t m,
                        int32_t *beats) {
  for (int64_t k = 0; k < m; k++) beats[k] = dbscan_beats(d[k], id[k], best_d[k], best_id[k]) ? 1 : 0;
}

// m (own, count) -> core[k] (0 / 1)
void dbscan_core_batch(const int32_t *own, const uint32_t *count, int32_t min_pts, int64_t m, int32_t *core) {
  for (int64_t k = 0; k < m; k++) core[k] = dbscan_core(own[k] != 0, count[k], min_pts) ? 1 : 0;
}

// the values of kind[]
void dbscan_kinds(int32_t out[3]) {
  out[0] = kDbNoise;
  out[1] = kDbBorder;
  out[2] = kDbCore;
}
}
