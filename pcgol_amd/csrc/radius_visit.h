// radius_visit.h -- how a kernel consumes a radius neighbourhood: one visitor over the three enumerations of
// range_enum.h, one query per lane.  normals.hip, mls.hip, keypoints.hip, fpfh.hip and boundary.hip enumerate through
// it; range.hip (counts, offsets, fills) and knearest.hip (a bound that shrinks) drive RowScan and the walks themselves.
//
// The contract, stated here and nowhere else:
//   * The set is every record p with ref_dist_sq(p, q) < bound, the bound STRICT, exactly what pcgx_kdtree_range_count
//     counts on that handle (a NaN query or bound: nothing).  take(p, d) is called for each member and for no other
//     record, d its float32 ref_dist_sq, p = {x, y, z, bits(id)}.
//   * Order: the grid's rows as grid_cover names them, z then y, a row's records ascending (kRangeGrid); the
//     reference's discovery order on the implicit tree (kRangeWalk) and on the patched tree (kRangeXWalk).  The
//     float64 sums of the consumers depend on it: the same call gives the same bits.
//   * Fat rows, grid only: a lane's first two rows of >= kRangeFatRow records are not its own work but the wave's.
//     After the lanes' own scans fat(owner, ox, oy, oz, rows) is called uniformly over the wave, once per set-aside row,
//     with the owner lane and the owner's query.  rows(each) runs THIS lane's share of that row, every 64th record from
//     its lane on, and calls each(p, d) for the records inside the bound of the owner's query.  What the caller does
//     with its share is its own: a partial accumulator, its reduction over the wave, the merge in the owner lane.
//   * So on the grid all 64 lanes of the wave must call radius_visit, and none may leave the kernel before it: a lane
//     with nothing to enumerate (no query, or nothing to do with one) passes live == false, scans nothing, owns no fat
//     row and shares in the others'.  On both walks a call with live == false does nothing, and a lane may return
//     before it.  `if (!live) return;` behind the call is right on every path.
//   * stk is this lane's column of the block's frame stack in LDS, [level][stk_stride] words: s_stack + threadIdx.x
//     with stk_stride the block size, the dynamic LDS sized by walk_stack_bytes / xwalk_stack_bytes (none on the grid).
//     Workgroups are one wave (kRangeWalkBlock), so threadIdx.x is the lane.
#pragma once
#include "knn_xwalk.h"
#include "range_walk.h"

namespace pcgx {

// Built inside the kernel from its arguments (a view the path does not use is never read).
struct RadiusViews {
  GridView g;
  TreeView tv;
  XTreeView xv;
  int64_t guard;  // xwalk_guard(Len())
};

template <int kSrc, class Take, class Fat>
__device__ __forceinline__ void radius_visit(const RadiusViews &V, uint32_t *stk, const int stk_stride, const float qx,
                                             const float qy, const float qz, const float bound, const bool live,
                                             Take &&take, Fat &&fat) {
  if constexpr (kSrc == kRangeGrid) {
    const uint32_t lane = threadIdx.x & 63u;
    grid_radius_scan(
        V.g, qx, qy, qz, bound, live,
        [&](const float4 &p) {
          const float d = ref_dist_sq(p.x, p.y, p.z, qx, qy, qz);
          if (d < bound) take(p, d);  // kdtree.go:166,178
        },
        [&](const int owner, const uint32_t rf, const uint32_t re, const float ox, const float oy, const float oz) {
          fat(owner, ox, oy, oz, [&](auto &&each) {
            for (uint32_t r = rf + lane; r < re; r += 64u) {
              const float4 p = V.g.pts[r];
              const float d = ref_dist_sq(p.x, p.y, p.z, ox, oy, oz);
              if (d < bound) each(p, d);
            }
          });
        });
  } else if (!live) {
    return;
  } else if constexpr (kSrc == kRangeWalk) {
    // (range_walk_nodes reports only DistSq < bound)
    range_walk_nodes<false>(V.tv, stk, stk_stride, qx, qy, qz, bound, [=]() { return bound; }, take);
  } else {
    auto hit = [&](const float4 &nd, const float d) {
      if (d < bound) take(nd, d);
      return true;
    };
    xwalk(V.xv, stk, stk_stride, qx, qy, qz, V.guard, [&]() { return bound; }, hit, hit);
  }
}

}  // namespace pcgx
