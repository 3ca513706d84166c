// range_enum.h -- the one enumeration of a radius neighbourhood: every point p with DistSq(p, q) < r*r.
//
// KDTree.Range (range.hip), surface normals (normals.hip), region growing (segment.hip) and Range on a handle that has
// seen DeletePoint all enumerate this set, and normals promise exactly the set pcgx_kdtree_range_count counts.  So
// what decides it is stated here once: the reference's float32 DistSq, which source a handle's Range takes
// (range_source), and the scan of the grid's cells with the wave-shared fat rows (grid_radius_scan).  The walks
// themselves are range_walk.h (implicit tree) and knn_xwalk.h (patched tree).
#pragma once
#include <stdlib.h>

#include "knn_grid.h"

namespace pcgx {

// The reference's DistSq in float32 (mat/vec3.go:18-20,38-40): (dx * dx + dy * dy) + dz * dz with d = p - q, never
// contracted (-ffp-contract=off on both sides)
__host__ __device__ __forceinline__ float ref_dist_sq(const float px, const float py, const float pz, const float qx,
                                                      const float qy, const float qz) {
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return (dx * dx + dy * dy) + dz * dz;
}

// Where a handle's neighbourhoods come from.  (An int template argument of the kernels: normals_kernel<kSrc>,
// range_kernel<kSrc, kFill>.)
enum RangeSrc { kRangeGrid = 0, kRangeWalk = 1, kRangeXWalk = 2 };

// PCGX_RANGE_WALK=1: the tree walk even where the handle has a grid (measurements, tests of the walk).  Read per call:
// the tests switch between the two.
inline bool range_walk_forced() {
  const char *e = getenv("PCGX_RANGE_WALK");
  return e && *e && *e != '0';
}

// A handle with deletions walks the reference's patched tree (knn_explicit.hip); else its grid, unless the walk is
// forced.  (PCGX_GRID does not apply: it is a switch of Nearest's certified path.)
inline RangeSrc range_source(const pcgx_kdtree *outer) {
  if (outer->n_deleted > 0) return kRangeXWalk;
  return outer->grid_ok && !range_walk_forced() ? kRangeGrid : kRangeWalk;
}

// A row of at least this many records (one site of the cloud taken thousands of times) is not one lane's work -- 25 ms
// of dependent loop for 100k records: the whole wave scans it.
constexpr uint32_t kRangeFatRow = 4096u;

// Every record of the cells grid_cover names for the lane's query (a NaN bound or query: the box is some cell or
// other, and no distance compares below the bound, as in the walk).  take(const float4 &p) is called for every record
// of the lane's own rows, four records in flight; the caller tests DistSq.  Up to two rows of >= kRangeFatRow records
// per lane are set aside, and then, uniformly over the wave, fat(owner, rf, re, ox, oy, oz) is called once for each
// such row [rf, re) of each owner lane with the owner's query: the caller shares the row out over the wave.  A third
// fat row is the lane's own work.  All 64 lanes of the wave must call this; a lane without a query passes live == false
// and scans nothing of its own.
template <class Take, class Fat>
__device__ __forceinline__ void grid_radius_scan(const GridView &g, const float qx, const float qy, const float qz,
                                                 const float bound, const bool live, Take &&take, Fat &&fat) {
  GridBox box = grid_cover(g, qx, qy, qz, bound);
  if (!live) box.z1 = box.z0 - 1;
  uint32_t fat_f0 = 0u, fat_e0 = 0u, fat_f1 = 0u, fat_e1 = 0u;
  int nfat = 0;
  for (int z = box.z0; z <= box.z1; z++) {
    for (int y = box.y0; y <= box.y1; y++) {
      const uint32_t row = ((uint32_t)z * (uint32_t)g.ny + (uint32_t)y) * (uint32_t)g.nx;
      uint32_t f = g.start[row + (uint32_t)box.x0];
      const uint32_t e = g.start[row + (uint32_t)box.x1 + 1u];
      if (e > f && e - f >= kRangeFatRow && nfat < 2) {
        if (nfat == 0) { fat_f0 = f; fat_e0 = e; }
        else { fat_f1 = f; fat_e1 = e; }
        nfat++;
        continue;
      }
      for (; f + 4u <= e; f += 4u) {  // four records in flight
        const float4 p0 = g.pts[f], p1 = g.pts[f + 1u], p2 = g.pts[f + 2u], p3 = g.pts[f + 3u];
        take(p0); take(p1); take(p2); take(p3);
      }
      for (; f < e; f++) take(g.pts[f]);
    }
  }
  if (__ballot(nfat > 0) == 0ull) return;
  for (int k = 0; k < 2; k++) {
    unsigned long long owners = __ballot(nfat > k);
    while (owners != 0ull) {  // uniform
      const int owner = __builtin_ctzll(owners);
      owners &= owners - 1ull;
      const float ox = __shfl(qx, owner), oy = __shfl(qy, owner), oz = __shfl(qz, owner);
      const uint32_t rf = __shfl(k == 0 ? fat_f0 : fat_f1, owner), re = __shfl(k == 0 ? fat_e0 : fat_e1, owner);
      fat(owner, rf, re, ox, oy, oz);
    }
  }
}

}  // namespace pcgx
