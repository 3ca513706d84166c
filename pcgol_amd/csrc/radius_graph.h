// radius_graph.h -- the connected components of the radius graph, one statement for region growing (segment.hip),
// cluster extraction (cluster.hip) and density clustering (dbscan.hip, through clusters_enqueue).  The vertices are the
// tree's points; an edge joins two points whose reference DistSq is strictly below the bound and which pass the
// feature's own test, an edge policy: a plain device struct, passed to the kernels by value, with
//   kWalks                 may it run on a handle without a grid?  (false: it reads nothing, and only a grid promises
//                          that every point is finite)
//   live(pos, id)          does this point take part at all?  If not it enumerates nothing and stays its own root.
//   mine(pos, id)          what it compares its neighbours with
//   joins(pos, id, mine)   is this neighbour inside the bound an edge?
// pos is the position the union-find works on: cell order on the grid, the id on the walk.  A component is a property of
// a set and the union-find (uf.h) does not care in which order it is told the edges, so the passes give the same roots
// whatever the policy; what a root is called, and what is counted under it, goes through wave_root_flush.
#pragma once
#include "knn_grid.h"
#include "range_walk.h"
#include "uf.h"

namespace pcgx {

// The slot's node, if it has one.
__device__ __forceinline__ bool tree_slot_node(const TreeView &tv, const uint32_t b, float4 *nd) {
  if (b >= (1u << tv.depth)) return false;
  const int depth = 31 - __clz((int)b);
  const uint32_t sz = node_size(b, depth, (uint32_t)tv.n + 1u);
  if (sz == 0u || sz > (uint32_t)tv.n) return false;
  *nd = node_at(tv.nodes, b);
  return true;
}

// The self scan: the lane of position f0 (the record me) enumerates the records of its own grid_cover, rows z then y,
// and calls each(f, p, d) for every record p at position f with d = DistSq(p, me) < bound.  kBelow clips every row at
// f0: each edge from its higher end.  One record at a time, and no wave-shared fat-row path (range_enum.h): a row of
// thousands of coincident points is one lane's loop for each of them.
template <bool kBelow, class Each>
__device__ __forceinline__ void grid_self_scan(const GridView &g, const int64_t f0, const float4 &me, const float bound,
                                               Each &&each) {
  const GridBox box = grid_cover(g, me.x, me.y, me.z, bound);
  for (int z = box.z0; z <= box.z1; z++) {
    for (int y = box.y0; y <= box.y1; y++) {
      GridRow r = grid_row(g, z, y, box.x0, box.x1);
      if (kBelow) r.e = r.e < (uint32_t)f0 ? r.e : (uint32_t)f0;
      for (uint32_t f = r.f; f < r.e; f++) {
        const float4 p = g.pts[f];
        const float d = ref_dist_sq(p.x, p.y, p.z, me.x, me.y, me.z);
        if (d < bound) each(f, p, d);
      }
    }
  }
}

// The components on a handle with a uniform grid (knn_grid.h).  Which points lie within the radius of a point does not
// depend on the walk (range.hip), and a union-find does not care in which order it is told the edges -- but it does
// care how many trees it has to merge and who merges them at the same time: the single pass of the walk's form below
// spends 370 of its 600 us at 300k points (region growing) in finds and compare-and-swap retries.  Here the union-find
// works on the points' positions in CELL ORDER (the grid's own order), one lane per point:
//  (1) kHookMin: every live point hooks itself under the joining neighbour with the SMALLEST position below its own (a
//      store to its own word: no contention, no find).  In cell order "smallest" means lowest z, then y, then x: the
//      trees are columns that run down through a component, and only points with nothing of their component below them
//      are roots -- hooked by point id, whose order has nothing to do with space, every sixth point was one;
//  (2) pointer jumping (uf_jump_kernel) makes every parent a root;
//  (3) else: a second pass over the neighbourhoods unions what is still apart (few trees, roots one hop away);
//  (4) the caller's: pointer jumping again, then roots -> the component's smallest point id (wave_root_flush).
template <bool kHookMin, class Edge>
__global__ __launch_bounds__(256) void rgraph_grid_kernel(GridView g, int64_t n, float bound, Edge edge,
                                                          uint32_t *__restrict__ parent) {
  const int64_t f0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f0 >= n) return;
  const float4 me = g.pts[f0];
  const uint32_t id0 = __float_as_uint(me.w);
  if (!edge.live((uint32_t)f0, id0)) return;  // (parent[f0] == f0 from the caller's init)
  const auto mine = edge.mine((uint32_t)f0, id0);
  uint32_t best = (uint32_t)f0;                                                // kHookMin: the lowest joining neighbour
  uint32_t my_root = kHookMin ? (uint32_t)f0 : uf_find(parent, (uint32_t)f0);  // else: a root this point was seen under
  grid_self_scan<true>(g, f0, me, bound, [&](const uint32_t f, const float4 &p, float) {
    if (!edge.joins(f, __float_as_uint(p.w), mine)) return;
    if (kHookMin)
      best = f < best ? f : best;
    else
      my_root = uf_link(parent, my_root, f);
  });
  if (kHookMin) parent[f0] = best;
}

// The walk's form, for a handle without a grid: one lane per tree node, the Range() neighbourhood of the node's point
// (range_walk.h), positions are ids.  Each undirected edge is seen from both ends (the distance expression is symmetric
// bit for bit); the larger id unions.
template <class Edge>
__global__ __launch_bounds__(kRangeWalkBlock) void rgraph_walk_kernel(TreeView tv, float bound, Edge edge,
                                                                      uint32_t *__restrict__ parent) {
  extern __shared__ uint32_t s_stack[];
  float4 nd;
  if (!tree_slot_node(tv, blockIdx.x * kRangeWalkBlock + threadIdx.x + 1u, &nd)) return;
  const int32_t id = __float_as_int(nd.w);
  if (!edge.live((uint32_t)id, (uint32_t)id)) return;
  const auto mine = edge.mine((uint32_t)id, (uint32_t)id);
  uint32_t my_root = (uint32_t)id;  // (a root this point was seen under: most neighbours are under it already)
  range_walk(tv, s_stack + threadIdx.x, kRangeWalkBlock, nd.x, nd.y, nd.z, bound, [&](int32_t j, float) {
    if (j < id && edge.joins((uint32_t)j, (uint32_t)j, mine)) my_root = uf_link(parent, my_root, (uint32_t)j);
  });
}

// The component passes up to, but not including, the last pointer jumping, which is the caller's: density clustering
// runs its border pass before it, and region growing's walk flattens instead.  parent[pos] == pos on entry; a is the
// tree the neighbourhoods come from, n its Len().
template <class Edge>
pcgx_status rgraph_components_enqueue(const pcgx_kdtree *a, bool on_grid, int64_t n, float bound, const Edge &edge,
                                      uint32_t *parent, hipStream_t st) {
  if (on_grid) {
    const dim3 nb((unsigned)((n + 255) / 256)), block(256);
    hipLaunchKernelGGL((rgraph_grid_kernel<true, Edge>), nb, block, 0, st, a->grid, n, bound, edge, parent);
    hipLaunchKernelGGL(uf_jump_kernel, nb, block, 0, st, parent, n);
    hipLaunchKernelGGL((rgraph_grid_kernel<false, Edge>), nb, block, 0, st, a->grid, n, bound, edge, parent);
  } else if constexpr (Edge::kWalks) {
    const TreeView tv = a->view();
    const uint32_t slots = 1u << tv.depth;
    hipLaunchKernelGGL(rgraph_walk_kernel<Edge>, dim3((slots + kRangeWalkBlock - 1) / kRangeWalkBlock),
                       dim3(kRangeWalkBlock), walk_stack_bytes(tv, kRangeWalkBlock), st, tv, bound, edge, parent);
  } else {
    return fail(PCGX_E_INVALID, "radius graph: this edge test needs a handle with a grid");
  }
  return PCGX_OK;
}

// One (root, count, smallest id) per lane -> memory; all 64 lanes call it, todo = the ballot of the valid ones.  The
// lanes of a wave are neighbours in space and mostly of one component: one atomic (with kCount a pair) per distinct
// root of the wave, and no atomicMin when the word already holds something smaller -- 150k atomicMin on the one word of
// a large region take 2 ms: same-address atomics are served one after the other.  Without kCount, cnt and count are
// not looked at.
template <bool kCount>
__device__ __forceinline__ void wave_root_flush(const bool valid, const uint32_t root, const uint32_t cnt, const uint32_t id,
                                                const int lane, unsigned long long todo, uint32_t *__restrict__ count,
                                                uint32_t *__restrict__ min_id) {
  while (todo) {  // uniform
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)root, leader);
    const bool mine = valid && root == r;
    const unsigned long long same = __ballot(mine);
    uint32_t m = mine ? id : 0xffffffffu, c = mine ? cnt : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t v = (uint32_t)__shfl_xor((int)m, o);
      m = v < m ? v : m;
      if (kCount) c += (uint32_t)__shfl_xor((int)c, o);
    }
    if (lane == leader) {
      if (kCount) atomicAdd(count + r, c);
      if (m < __atomic_load_n(min_id + r, __ATOMIC_RELAXED)) atomicMin(min_id + r, m);
    }
    todo &= ~same;
  }
}

}  // namespace pcgx
