// dbscan.hip -- density clustering (DBSCAN) over the tree's own points, and the core flag radius outlier removal keeps
// by (extension: no reference parity; include/pcgx.h, "density clusters" and pcgx_ror_filter).
//
// One fact per point carries both calls: does N(i), the set Range counts, hold at least min_pts points?  Everything
// else is cluster extraction's (cluster.hip): the component passes run on the core flags where they ran on the usable
// flags, and sizes, names, ranking and grouping are its tail, reached through clusters_enqueue (dbscan.h), one body.
//
// The two passes that are new, both one lane per point in the grid's cell order (the walk's form for a handle without a
// grid: one lane per tree node, positions are ids):
//   flag pass    counts the members of N(i) and writes the core flag as a byte beside the cell-ordered points, where
//                rgraph_grid_kernel<., ClusterEdge<kCutFlags>> reads a byte per candidate.  Only the flag leaves the
//                pass, so with kStop a lane stops counting at min_pts (DESIGN.md 3.21 has both forms' times).
//   border pass  a usable lane that is not core enumerates its whole neighbourhood -- not only the positions below its
//                own: its nearest core neighbour may lie on either side -- keeps the smallest (DistSq, id) among the core
//                candidates (dbscan_terms.h) and stores that position into its own parent word.  A store to the lane's
//                own word, as in the hook pass, and nobody hooks under a border point: it carries no edge.  The pointer
//                jumping that follows takes it to its component's root.
// No atomics at all here, no scratch; no wave-shared fat-row path, as in the radius graph's self scan
// (radius_graph.h), which the border pass takes whole (with kStop the flag pass leaves a fat row after min_pts records).
#include <math.h>
#include <stdlib.h>

#include "dbscan.h"
#include "dbscan_terms.h"
#include "knn_grid.h"
#include "radius_graph.h"

namespace pcgx {

// ------------------------------------------------------------------ flag pass
template <bool kStop>
__global__ __launch_bounds__(256) void db_flag_grid_kernel(GridView g, int64_t n, float bound, int32_t min_pts,
                                                           uint8_t *__restrict__ core) {
  const int64_t f0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f0 >= n) return;
  const float4 me = g.pts[f0];
  const bool own = ref_dist_sq(me.x, me.y, me.z, me.x, me.y, me.z) < bound;  // i in N(i)
  uint32_t cnt = 0u;
  bool more = true;
  GridBox box = grid_cover(g, me.x, me.y, me.z, bound);
  if (!own) box.z1 = box.z0 - 1;  // an unusable point has nobody in reach
  for (int z = box.z0; more && z <= box.z1; z++) {
    for (int y = box.y0; more && y <= box.y1; y++) {
      const GridRow r = grid_row(g, z, y, box.x0, box.x1);
      uint32_t f = r.f;
      const uint32_t e = r.e;
      // with the stop: four records in flight (range_enum.h's RowScan) and the stop looked at once per four -- tested
      // per record it cost more where it never fires than it saved where it does.  Without it the plain loop below is
      // the whole scan: the compiler pipelines it better than the four written out (DESIGN.md 3.21 has the figures)
      for (; kStop && more && f + 4u <= e; f += 4u) {
        const float4 p0 = g.pts[f], p1 = g.pts[f + 1u], p2 = g.pts[f + 2u], p3 = g.pts[f + 3u];
        cnt += (ref_dist_sq(p0.x, p0.y, p0.z, me.x, me.y, me.z) < bound ? 1u : 0u) +
               (ref_dist_sq(p1.x, p1.y, p1.z, me.x, me.y, me.z) < bound ? 1u : 0u) +
               (ref_dist_sq(p2.x, p2.y, p2.z, me.x, me.y, me.z) < bound ? 1u : 0u) +
               (ref_dist_sq(p3.x, p3.y, p3.z, me.x, me.y, me.z) < bound ? 1u : 0u);
        more = (int64_t)cnt < (int64_t)min_pts;
      }
      for (; more && f < e; f++) {
        const float4 p = g.pts[f];
        cnt += ref_dist_sq(p.x, p.y, p.z, me.x, me.y, me.z) < bound ? 1u : 0u;
      }
      if (kStop) more = (int64_t)cnt < (int64_t)min_pts;
    }
  }
  core[f0] = dbscan_core(own, cnt, min_pts) ? (uint8_t)1 : (uint8_t)0;
}

// The walk's form: the whole count (the walk has no way out before its end).
__global__ __launch_bounds__(kRangeWalkBlock) void db_flag_walk_kernel(TreeView tv, float bound, int32_t min_pts,
                                                                       uint8_t *__restrict__ core) {
  extern __shared__ uint32_t s_stack[];
  float4 nd;
  if (!tree_slot_node(tv, blockIdx.x * kRangeWalkBlock + threadIdx.x + 1u, &nd)) return;
  const bool own = ref_dist_sq(nd.x, nd.y, nd.z, nd.x, nd.y, nd.z) < bound;
  if (!own) return;  // (core[] was zeroed)
  uint32_t cnt = 0u;
  range_walk(tv, s_stack + threadIdx.x, kRangeWalkBlock, nd.x, nd.y, nd.z, bound, [&](int32_t, float) { cnt++; });
  core[__float_as_uint(nd.w)] = dbscan_core(own, cnt, min_pts) ? (uint8_t)1 : (uint8_t)0;
}

// ------------------------------------------------------------------ border pass
__global__ __launch_bounds__(256) void db_border_grid_kernel(GridView g, int64_t n, float bound,
                                                             const uint8_t *__restrict__ core, uint8_t *__restrict__ kindp,
                                                             uint32_t *__restrict__ parent) {
  const int64_t f0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f0 >= n) return;
  if (core[f0]) {
    kindp[f0] = kDbCore;
    return;
  }
  const float4 me = g.pts[f0];
  float best_d = __builtin_inff();
  uint32_t best_id = 0xffffffffu, best_f = (uint32_t)f0;
  // (an unusable point is no border point: no distance from it compares below the bound)
  grid_self_scan<false>(g, f0, me, bound, [&](const uint32_t f, const float4 &p, const float d) {
    // a statement of its own: written as `core[f] && dbscan_beats(...)` the record's 16-byte load became a 12-byte one
    // and a dependent read of the id per core candidate, 8 us of 655 where nearly every point is a border point
    if (!core[f]) return;
    const uint32_t id = __float_as_uint(p.w);
    if (dbscan_beats(d, id, best_d, best_id)) {
      best_d = d;
      best_id = id;
      best_f = f;
    }
  });
  const bool border = best_f != (uint32_t)f0;
  kindp[f0] = border ? kDbBorder : kDbNoise;
  if (border) parent[f0] = best_f;
}

__global__ __launch_bounds__(kRangeWalkBlock) void db_border_walk_kernel(TreeView tv, float bound,
                                                                         const uint8_t *__restrict__ core,
                                                                         uint8_t *__restrict__ kindp,
                                                                         uint32_t *__restrict__ parent) {
  extern __shared__ uint32_t s_stack[];
  float4 nd;
  if (!tree_slot_node(tv, blockIdx.x * kRangeWalkBlock + threadIdx.x + 1u, &nd)) return;
  const uint32_t id0 = __float_as_uint(nd.w);
  if (core[id0]) {
    kindp[id0] = kDbCore;
    return;
  }
  if (!(ref_dist_sq(nd.x, nd.y, nd.z, nd.x, nd.y, nd.z) < bound)) return;  // (kindp[] was zeroed)
  float best_d = __builtin_inff();
  uint32_t best_id = 0xffffffffu;
  range_walk(tv, s_stack + threadIdx.x, kRangeWalkBlock, nd.x, nd.y, nd.z, bound, [&](int32_t j, float d) {
    if (core[j] && dbscan_beats(d, (uint32_t)j, best_d, best_id)) {
      best_d = d;
      best_id = (uint32_t)j;
    }
  });
  if (best_id == 0xffffffffu) return;
  kindp[id0] = kDbBorder;
  parent[id0] = best_id;  // positions are ids
}

// ------------------------------------------------------------------ by id
__global__ __launch_bounds__(256) void db_kind_kernel(const float4 *__restrict__ pts, int64_t n,
                                                      const uint8_t *__restrict__ kindp, int32_t all_core,
                                                      uint8_t *__restrict__ kind) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  const uint32_t id = pts ? __float_as_uint(pts[f].w) : (uint32_t)f;
  const uint8_t k = kindp[f];
  kind[id] = k != 0 && all_core ? (uint8_t)kDbCore : k;
}

void dbscan_flags_launch(const pcgx_kdtree *a, bool on_grid, int64_t n, float bound, int32_t min_pts, bool count_all,
                         uint8_t *core, hipStream_t st) {
  if (on_grid) {
    const unsigned nb = (unsigned)((n + 255) / 256);
    if (count_all)
      hipLaunchKernelGGL(db_flag_grid_kernel<false>, dim3(nb), dim3(256), 0, st, a->grid, n, bound, min_pts, core);
    else
      hipLaunchKernelGGL(db_flag_grid_kernel<true>, dim3(nb), dim3(256), 0, st, a->grid, n, bound, min_pts, core);
    return;
  }
  const TreeView tv = a->view();
  const uint32_t slots = 1u << tv.depth;
  hipLaunchKernelGGL(db_flag_walk_kernel, dim3((slots + kRangeWalkBlock - 1) / kRangeWalkBlock), dim3(kRangeWalkBlock),
                     walk_stack_bytes(tv, kRangeWalkBlock), st, tv, bound, min_pts, core);
}

void dbscan_border_launch(const pcgx_kdtree *a, bool on_grid, int64_t n, float bound, const uint8_t *core, uint8_t *kindp,
                          uint32_t *parent, hipStream_t st) {
  if (on_grid) {
    hipLaunchKernelGGL(db_border_grid_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a->grid, n, bound, core,
                       kindp, parent);
    return;
  }
  const TreeView tv = a->view();
  const uint32_t slots = 1u << tv.depth;
  hipLaunchKernelGGL(db_border_walk_kernel, dim3((slots + kRangeWalkBlock - 1) / kRangeWalkBlock), dim3(kRangeWalkBlock),
                     walk_stack_bytes(tv, kRangeWalkBlock), st, tv, bound, core, kindp, parent);
}

void dbscan_kind_launch(const float4 *pts, int64_t n, const uint8_t *kindp, bool all_core, uint8_t *kind, hipStream_t st) {
  hipLaunchKernelGGL(db_kind_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pts, n, kindp,
                     all_core ? 1 : 0, kind);
}

// PCGX_DBSCAN_COUNT_ALL=1: the flag pass without the early stop (measurements).  Read per call.
static bool dbscan_count_all() {
  const char *e = getenv("PCGX_DBSCAN_COUNT_ALL");
  return e && *e && *e != '0';
}

pcgx_status dbscan_core_by_id_enqueue(const pcgx_kdtree *t, float radius, int32_t min_pts, uint8_t *d_core_by_id,
                                      hipStream_t st) {
  const int64_t n = t->n;
  const float bound = radius * radius;
  const bool on_grid = t->grid_ok && !range_walk_forced();
  if (!on_grid) {
    PCGX_HIP_TRY(hipMemsetAsync(d_core_by_id, 0, (size_t)n, st));
    dbscan_flags_launch(t, false, n, bound, min_pts, dbscan_count_all(), d_core_by_id, st);
  } else {
    uint8_t *core = nullptr;
    PCGX_TRY(ctx().arena.alloc_n((size_t)n, &core));
    dbscan_flags_launch(t, true, n, bound, min_pts, dbscan_count_all(), core, st);
    dbscan_kind_launch(t->grid.pts, n, core, false, d_core_by_id, st);
  }
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

}  // namespace pcgx

using namespace pcgx;

namespace {

pcgx_status dbscan_check(const char *fn, const pcgx_kdtree *t, float radius, int32_t min_pts, int64_t min_size,
                         int64_t max_size, const void *labels, const void *n_clusters) {
  PCGX_TRY(clusters_check(fn, t, radius, nullptr, 0.0f, nullptr, 0.0f, min_size, max_size, labels, n_clusters));
  if (min_pts < 1) return fail(PCGX_E_INVALID, "%s: min_pts must be >= 1", fn);
  return PCGX_OK;
}

}  // namespace

extern "C" pcgx_status pcgx_kdtree_dbscan_dev(const pcgx_kdtree *t, float radius, int32_t min_pts, int64_t min_size,
                                              int64_t max_size, int32_t *d_labels, int32_t *d_n_clusters, int32_t *d_sizes,
                                              int32_t *d_ids, uint8_t *d_kind, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(dbscan_check("pcgx_kdtree_dbscan_dev", t, radius, min_pts, min_size, max_size, d_labels, d_n_clusters));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  const int64_t n = t->n;
  if (n == 0) {
    if (d_n_clusters) PCGX_HIP_TRY(hipMemsetAsync(d_n_clusters, 0, sizeof(int32_t), st));
    return PCGX_OK;
  }
  const pcgx_kdtree *a = nullptr;
  bool empty = false;
  PCGX_TRY(resolve_tree(t, &a, &empty));  // after DeletePoint: the tree over the remaining points, original ids
  PCGX_TRY(ctx().arena.begin(st));
  const ClusterDensity density{min_pts, dbscan_count_all(), d_kind};
  return clusters_enqueue(empty ? nullptr : a, n, radius, nullptr, 0.0f, 0, nullptr, 0.0f, min_size, max_size, &density,
                          d_labels, d_n_clusters, d_sizes, d_ids, st);
}

extern "C" pcgx_status pcgx_kdtree_dbscan(const pcgx_kdtree *t, float radius, int32_t min_pts, int64_t min_size,
                                          int64_t max_size, int64_t *labels, int64_t *n_clusters, int64_t *sizes,
                                          int64_t *ids, uint8_t *kind) {
  PCGX_API_CALL();
  PCGX_TRY(dbscan_check("pcgx_kdtree_dbscan", t, radius, min_pts, min_size, max_size, labels, n_clusters));
  const int64_t n = t->n;
  if (n == 0) {
    if (n_clusters) *n_clusters = 0;
    return PCGX_OK;
  }
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  int32_t *d_out = nullptr;  // labels [n], sizes [n], ids [n], the count
  uint8_t *d_kind = nullptr;
  PCGX_TRY(ha.alloc_n((size_t)n * 3 + 1, &d_out));
  if (kind) PCGX_TRY(ha.alloc_n((size_t)n, &d_kind));
  PCGX_TRY(pcgx_kdtree_dbscan_dev(t, radius, min_pts, min_size, max_size, d_out, d_out + 3 * n, sizes ? d_out + n : nullptr,
                                  ids ? d_out + 2 * n : nullptr, d_kind, st));
  RawVector<int32_t> h((size_t)n * 3 + 1);
  PCGX_TRY(staged_download(h.data(), d_out, ((size_t)n * 3 + 1) * 4, st));
  if (kind) PCGX_TRY(staged_download(kind, d_kind, (size_t)n, st));
  for (int64_t i = 0; i < n; i++) labels[i] = h[(size_t)i];
  if (sizes)
    for (int64_t i = 0; i < n; i++) sizes[i] = h[(size_t)(n + i)];
  if (ids)
    for (int64_t i = 0; i < n; i++) ids[i] = h[(size_t)(2 * n + i)];
  *n_clusters = h[(size_t)(3 * n)];
  return PCGX_OK;
}
