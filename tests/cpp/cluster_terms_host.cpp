// csrc/cluster_terms.h on the host (tests/test_cluster_terms_host.py): the expressions the kernels compile, over
// batches, through extern "C".
#include <stdint.h>

#include "cluster_terms.h"

using namespace pcgx;

extern "C" {

// m points -> usable[k] (0 / 1).  own[k]: the point is in its own neighbourhood; normals / curvature may be NULL
void cluster_usable_batch(const int32_t *own, const float *normals, const float *curvature, float max_curvature, int64_t m,
                          int32_t *usable) {
  for (int64_t k = 0; k < m; k++)
    usable[k] = cluster_usable(own[k] != 0, normals != nullptr, normals ? normals[3 * k] : 0.0f,
                               normals ? normals[3 * k + 1] : 0.0f, normals ? normals[3 * k + 2] : 0.0f,
                               curvature != nullptr, curvature ? curvature[k] : 0.0f, max_curvature)
                    ? 1 : 0;
}

// m pairs of normals -> agree[k] (0 / 1)
void cluster_agree_batch(const float *ni, const float *nj, float min_cos, int32_t oriented, int64_t m, int32_t *agree) {
  for (int64_t k = 0; k < m; k++)
    agree[k] = cluster_normals_agree(ni[3 * k], ni[3 * k + 1], ni[3 * k + 2], nj[3 * k], nj[3 * k + 1], nj[3 * k + 2], min_cos,
                                     oriented) ? 1 : 0;
}

// m (is_seed, size) -> key[k], and the size a seed's key gives back
void cluster_key_batch(const int32_t *is_seed, const uint32_t *size, uint32_t n, int64_t min_size, int64_t max_size, int64_t m,
                       uint32_t *key, uint32_t *size_back) {
  for (int64_t k = 0; k < m; k++) {
    key[k] = cluster_seed_key(is_seed[k] != 0, size[k], n, min_size, max_size);
    size_back[k] = cluster_key_size(key[k], n);
  }
}
}
