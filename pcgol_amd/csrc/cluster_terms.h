// cluster_terms.h -- the decisions of cluster extraction, shared by the device kernels (cluster.hip) and the host test
// (tests/cpp/cluster_terms_host.cpp): one expression, compiled by both.
// NOT in the reference: no parity, checked against the NumPy oracle's restatement (tests/cluster_oracle.py).
//
// Contract (include/pcgx.h, "clusters"): the dot product of two normals in float64 from the float32 components, the
// products exact, the two additions rounded in this order, nothing fused (build with -ffp-contract=off, the rule of
// ref_dist_sq).
#pragma once
#include "pcgx_math.h"

namespace pcgx {

PCGX_HD bool cluster_finite(const float v) {
  uint32_t b;
  __builtin_memcpy(&b, &v, 4);
  return (b & 0x7f800000u) != 0x7f800000u;
}

// May a point carry this normal?  Its three components finite and not all zero (the zero normal is what
// pcgx_kdtree_normals answers for a degenerate neighbourhood).
PCGX_HD bool cluster_normal_ok(const float nx, const float ny, const float nz) {
  return cluster_finite(nx) && cluster_finite(ny) && cluster_finite(nz) && !(nx == 0.0f && ny == 0.0f && nz == 0.0f);
}

// May a point of this curvature take part?  A NaN fails.
PCGX_HD bool cluster_curvature_ok(const float curvature, const float max_curvature) { return curvature <= max_curvature; }

// The usable-point test.  in_own_neighbourhood: DistSq(point, point) < radius^2 for a point the handle still holds
// (false for a deleted id and for a NaN or infinite coordinate).  has_normals / has_curvature: the arrays were given.
PCGX_HD bool cluster_usable(const bool in_own_neighbourhood, const bool has_normals, const float nx, const float ny,
                            const float nz, const bool has_curvature, const float curvature, const float max_curvature) {
  return in_own_neighbourhood && (!has_normals || cluster_normal_ok(nx, ny, nz)) &&
         (!has_curvature || cluster_curvature_ok(curvature, max_curvature));
}

// Do the normals of two usable points agree?  Symmetric in (i, j) bit for bit: each product and the first sum commute.
PCGX_HD bool cluster_normals_agree(const float nxi, const float nyi, const float nzi, const float nxj, const float nyj,
                                   const float nzj, const float min_cos, const int32_t oriented) {
  const double c = ((double)nxi * (double)nxj + (double)nyi * (double)nyj) + (double)nzi * (double)nzj;
  return oriented ? c >= (double)min_cos : fabs(c) >= (double)min_cos;
}

// Is a component of this size a cluster?  min_size <= 0 counts as 1; max_size == 0: no upper limit.
PCGX_HD bool cluster_size_kept(const uint32_t size, const int64_t min_size, const int64_t max_size) {
  const int64_t lo = min_size > 1 ? min_size : 1;
  return (int64_t)size >= lo && (max_size <= 0 || (int64_t)size <= max_size);
}

// The sort key of a point of a cloud of n points: n - size for the smallest id of a kept component (its seed), else n.
// A stable sort of the keys by id puts the seeds first, by decreasing size, equal sizes by ascending id; size >= 1, so no
// seed's key is n, and the keys need only the bits of n.
PCGX_HD uint32_t cluster_seed_key(const bool is_seed, const uint32_t size, const uint32_t n, const int64_t min_size,
                                  const int64_t max_size) {
  return is_seed && cluster_size_kept(size, min_size, max_size) ? n - size : n;
}
PCGX_HD uint32_t cluster_key_size(const uint32_t key, const uint32_t n) { return n - key; }

}  // namespace pcgx
