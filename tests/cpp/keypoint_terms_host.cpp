// csrc/keypoint_terms.h on the host (tests/test_keypoint_terms_host.py): the expressions the kernels compile, over
// batches, through extern "C".
#include <stdint.h>

#include "keypoint_terms.h"

using namespace pcgx;

extern "C" {

// m eigenvalue triples -> saliency[i]
void keypoint_saliency_batch(const float *eig, int64_t m, float gamma_21, float gamma_32, float *saliency) {
  for (int64_t i = 0; i < m; i++) saliency[i] = iss_saliency(eig[3 * i], eig[3 * i + 1], eig[3 * i + 2], gamma_21, gamma_32);
}

// m pairs (neighbour j, point i) -> beats[k] (0 / 1)
void keypoint_beats_batch(const float *sj, const int64_t *j, const float *si, const int64_t *i, int64_t m, int32_t *beats) {
  for (int64_t k = 0; k < m; k++) beats[k] = keypoint_beats(sj[k], j[k], si[k], i[k]) ? 1 : 0;
}

// m scores -> candidate[k] (0 / 1)
void keypoint_candidate_batch(const float *s, int64_t m, int32_t *cand) {
  for (int64_t k = 0; k < m; k++) cand[k] = keypoint_candidate(s[k]) ? 1 : 0;
}
}
