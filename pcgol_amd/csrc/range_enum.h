// range_enum.h -- the one enumeration of a radius neighbourhood: every point p with DistSq(p, q) < r*r.
//
// KDTree.Range (range.hip), surface normals (normals.hip), region growing (segment.hip), k nearest neighbours
// (knearest.hip) and Range on a handle that has seen DeletePoint all enumerate this set, and normals promise exactly the
// set pcgx_kdtree_range_count counts.  So what decides it is stated here once: the reference's float32 DistSq, which
// source a handle's Range takes (range_source), the scan of the grid's rows with the wave-shared fat rows (grid_row,
// RowScan, grid_radius_scan), and where a kernel's queries come from (QuerySource, query_source).  The walks
// themselves are range_walk.h (implicit tree) and knn_xwalk.h (patched tree); radius_visit.h puts the three behind
// one visitor for the kernels that only consume the set (normals, MLS, keypoints, FPFH).
#pragma once
#include <stdlib.h>

#include "knn_grid.h"

namespace pcgx {

// (ref_dist_sq, the reference's float32 DistSq, is pcgx_math.h's: the host programs of the tests compile it too)

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

// The records [f, e) of the cells x0 .. x1 (inclusive) of the grid's row (z, y).
struct GridRow {
  uint32_t f, e;
};
__device__ __forceinline__ GridRow grid_row(const GridView &g, const int z, const int y, const int x0, const int x1) {
  const uint32_t row = ((uint32_t)z * (uint32_t)g.ny + (uint32_t)y) * (uint32_t)g.nx;
  return GridRow{g.start[row + (uint32_t)x0], g.start[row + (uint32_t)x1 + 1u]};
}

// One lane's scan of grid rows.  row() calls take(const float4 &p) for every record of a row, in order, kInFlight (4 or
// 1) records loaded at a time, except that the lane's first two rows of >= kRangeFatRow records are set aside; a third
// fat row is the lane's own work.  Then share(), uniformly over the wave (all 64 lanes call it), calls fat(owner, rf, re, ox, oy, oz) once for
// each set-aside row [rf, re) of each owner lane with the owner's query: the caller shares the row out over the wave.
struct RowScan {
  uint32_t f0 = 0u, e0 = 0u, f1 = 0u, e1 = 0u;
  int nfat = 0;

  template <int kInFlight = 4, class Take>
  __device__ __forceinline__ void row(const GridView &g, const GridRow r, Take &&take) {
    static_assert(kInFlight == 4 || kInFlight == 1, "four records in flight, or one");
    uint32_t f = r.f;
    const uint32_t e = r.e;
    if (e > f && e - f >= kRangeFatRow && nfat < 2) {
      if (nfat == 0) { f0 = f; e0 = e; }
      else { f1 = f; e1 = e; }
      nfat++;
      return;
    }
    if constexpr (kInFlight == 4) {
      for (; f + 4u <= e; f += 4u) {
        const float4 p0 = g.pts[f], p1 = g.pts[f + 1u], p2 = g.pts[f + 2u], p3 = g.pts[f + 3u];
        take(p0); take(p1); take(p2); take(p3);
      }
    }
    for (; f < e; f++) take(g.pts[f]);
  }

  template <class Fat>
  __device__ __forceinline__ void share(const float qx, const float qy, const float qz, Fat &&fat) const {
    if (__ballot(nfat > 0) == 0ull) return;
    for (int k = 0; k < 2; k++) {
      unsigned long long owners = __ballot(nfat > k);
      while (owners != 0ull) {  // uniform
        const int owner = __builtin_ctzll(owners);
        owners &= owners - 1ull;
        const float ox = __shfl(qx, owner), oy = __shfl(qy, owner), oz = __shfl(qz, owner);
        const uint32_t rf = __shfl(k == 0 ? f0 : f1, owner), re = __shfl(k == 0 ? e0 : e1, owner);
        fat(owner, rf, re, ox, oy, oz);
      }
    }
  }
};

// Every record of the cells grid_cover names for the lane's query (a NaN bound or query: the box is some cell or
// other, and no distance compares below the bound, as in the walk), row by row through RowScan; the caller tests
// DistSq.  All 64 lanes of the wave must call this; a lane without a query passes live == false and scans nothing of
// its own.
template <class Take, class Fat>
__device__ __forceinline__ void grid_radius_scan(const GridView &g, const float qx, const float qy, const float qz,
                                                 const float bound, const bool live, Take &&take, Fat &&fat) {
  GridBox box = grid_cover(g, qx, qy, qz, bound);
  if (!live) box.z1 = box.z0 - 1;
  RowScan rows;
  for (int z = box.z0; z <= box.z1; z++)
    for (int y = box.y0; y <= box.y1; y++) rows.row(g, grid_row(g, z, y, box.x0, box.x1), take);
  rows.share(qx, qy, qz, fat);
}

// Where a kernel's queries come from: own[pos] ({x, y, z, bits(id)}: the tree's own points in the grid's cell order,
// where neighbouring lanes read the same cells), else q[perm[pos]] (perm: a Morton order, or none).  Results are
// written at the query's index / point id.
struct QuerySource {
  const float *q;
  const int32_t *perm;
  const float4 *own;
  int64_t nq;
};

// The query at launch position pos < nq: its index (point id) i and its coordinates.
__device__ __forceinline__ void read_query(const QuerySource &Q, const int64_t pos, int64_t &i, float &qx, float &qy,
                                           float &qz) {
  if (Q.own) {
    const float4 r = Q.own[pos];
    i = (int64_t)__float_as_uint(r.w);
    qx = r.x; qy = r.y; qz = r.z;
  } else {
    i = Q.perm ? (int64_t)Q.perm[pos] : pos;
    qx = Q.q[3 * i]; qy = Q.q[3 * i + 1]; qz = Q.q[3 * i + 2];
  }
}

// Caller batches from this size on run in Morton order.
constexpr int64_t kPresortMin = 16384;

// The nq queries at d_q, or (d_q == nullptr) the tree's own points, Len() of them, deleted ones included: in cell order
// where t has a grid, else by id (the patched tree's copy where src is kRangeXWalk -- xtree_view made it --, else
// gathered out of the tree's nodes); queries by index are put in Morton order from kPresortMin on.  Temporaries from
// ctx().arena, which the caller has begun.  (range.hip)
pcgx_status query_source(const pcgx_kdtree *t, RangeSrc src, const float *d_q, int64_t nq, QuerySource *Q,
                         hipStream_t st);

// *out = the map point id -> BFS slot of its node in the handle's implicit tree, made once per handle on first use (on
// st, which it then waits for: callers on other streams use it unordered; range.hip).  k-NN covariances fetch their
// neighbours' xyz by id through it.
pcgx_status range_inverse_map(const pcgx_kdtree *t, const uint32_t **out, hipStream_t st);

// q == NULL asks for the tree's own points: then nq must be Len().
inline pcgx_status own_query_check(const char *fn, const pcgx_kdtree *t, const float *q, const int64_t nq) {
  if (!q && nq != t->n) return fail(PCGX_E_INVALID, "%s: q == NULL takes the tree's own points: nq must equal Len()", fn);
  return PCGX_OK;
}

}  // namespace pcgx
