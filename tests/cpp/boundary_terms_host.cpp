// csrc/boundary_terms.h on the host (tests/test_boundary_terms_host.py): the expressions the kernel compiles, over
// batches, through extern "C".
#include <stdint.h>

#include "boundary_terms.h"

using namespace pcgx;

extern "C" {

// {sectors}, and T[1..15]
void boundary_constants(int32_t *sectors, double *tans) {
  *sectors = kBoundarySectors;
  for (int k = 0; k < 16; k++) tans[k] = boundary_tan(k);
}

// m normals -> usable[i] (0 / 1), frame[6 i ..] = {u, v}
void boundary_frame_batch(const float *n, int64_t m, int32_t *usable, double *frame) {
  for (int64_t i = 0; i < m; i++) {
    usable[i] = boundary_normal_usable(n[3 * i], n[3 * i + 1], n[3 * i + 2]) ? 1 : 0;
    const BoundaryFrame f = boundary_frame(n[3 * i], n[3 * i + 1], n[3 * i + 2]);
    const double o[6] = {f.ux, f.uy, f.uz, f.vx, f.vy, f.vz};
    for (int k = 0; k < 6; k++) frame[6 * i + k] = o[k];
  }
}

// m (met, usable, count, min_neighbors) -> evaluated[i] (0 / 1)
void boundary_evaluated_batch(const int32_t *met, const int32_t *usable, const int32_t *count, const int32_t *min_neighbors,
                              int64_t m, int32_t *evaluated) {
  for (int64_t i = 0; i < m; i++)
    evaluated[i] = boundary_evaluated(met[i] != 0, usable[i] != 0, count[i], min_neighbors[i]) ? 1 : 0;
}

// m pairs (normal, neighbour p, query q) -> ab[2 i ..], sector[i] (-1: none)
void boundary_direction_batch(const float *n, const float *p, const float *q, int64_t m, double *ab, int32_t *sector) {
  for (int64_t i = 0; i < m; i++) {
    const BoundaryFrame f = boundary_frame(n[3 * i], n[3 * i + 1], n[3 * i + 2]);
    boundary_direction(f, p[3 * i], p[3 * i + 1], p[3 * i + 2], q[3 * i], q[3 * i + 1], q[3 * i + 2], ab[2 * i], ab[2 * i + 1]);
    sector[i] = boundary_sector(ab[2 * i], ab[2 * i + 1]);
  }
}

// m directions (a, b) -> sector[i]
void boundary_sector_batch(const double *a, const double *b, int64_t m, int32_t *sector) {
  for (int64_t i = 0; i < m; i++) sector[i] = boundary_sector(a[i], b[i]);
}

// m masks -> gap[i]
void boundary_gap_batch(const uint64_t *mask, int64_t m, int32_t *gap) {
  for (int64_t i = 0; i < m; i++) gap[i] = boundary_gap(mask[i]);
}
}
