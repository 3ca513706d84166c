// dbscan_terms.h -- the decisions of density clustering, shared by the device kernels (dbscan.hip) and the host test
// (tests/cpp/dbscan_terms_host.cpp): one expression, compiled by both.
// NOT in the reference: no parity, checked against the NumPy oracle's restatement (tests/dbscan_oracle.py).
//
// Contract (include/pcgx.h, "density clusters"): a point is core when it is usable and its neighbourhood, itself
// included, holds at least min_pts points; a border point goes with the core neighbour of the smallest float32 DistSq,
// equal ones by the smallest id.
#pragma once
#include "pcgx_math.h"

namespace pcgx {

// what pcgx_kdtree_dbscan writes into kind[]
enum DbscanKind : uint8_t { kDbNoise = 0, kDbBorder = 1, kDbCore = 2 };

// The core test.  in_own_neighbourhood: DistSq(point, point) < radius^2 for a point the handle still holds;
// count: |N(i)|, or any lower bound of it that has reached min_pts (a count may stop there).
PCGX_HD bool dbscan_core(const bool in_own_neighbourhood, const uint32_t count, const int32_t min_pts) {
  return in_own_neighbourhood && (int64_t)count >= (int64_t)min_pts;
}

// Does the core candidate (d, id) beat the best so far (best_d, best_id)?  The smaller DistSq, equal ones (-0 == +0)
// by the smaller id; a NaN distance beats nobody, and nobody beats itself.
PCGX_HD bool dbscan_beats(const float d, const uint32_t id, const float best_d, const uint32_t best_id) {
  return d < best_d || (d == best_d && id < best_id);
}

}  // namespace pcgx
