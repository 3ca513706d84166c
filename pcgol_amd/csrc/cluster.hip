// cluster.hip -- cluster extraction: the connected components of the radius graph, optionally cut where the normals turn
// or the curvature is high, kept inside a size range, ranked and grouped (extension: no reference parity;
// include/pcgx.h, "clusters").
//
// What a user does after the ground plane is out: cut the rest into objects (PCL's EuclideanClusterExtraction) or into
// smooth faces.  A component is a property of a set, so nothing here depends on the order in which edges are met.
//
// Stages, all on the caller's stream, no count known to the host:
//   staging     one gather: the usable flag of every point (cluster_terms.h) as a byte, and with normals a
//               {nx, ny, nz, usable} record, BESIDE the grid's cell-ordered points (by id for a handle without a grid).
//               The inner loops below read positions, not ids (what reads by id cost) -- and nothing at
//               all in the Euclidean form on a grid, whose points are all finite and so all usable.
//   components  the radius graph's passes (radius_graph.h, with their measured reasons) under ClusterEdge: in cell order
//               every usable point hooks itself under the smallest qualifying position below its own, pointer jumping, a
//               union pass over what is still apart, jumping again.  Every edge from its higher end.  A handle without a
//               grid (PCGX_RANGE_WALK=1, after DeletePoint: the rebuilt tree of resolve_tree) takes the walk's form of
//               the same union, positions = ids.
//   sizes and   per root the number of usable points under it and their smallest id, one atomic per distinct root of a
//   names       wave (wave_root_flush); then every point's name (the smallest id), size and sort key.
//   ranking     one stable radix sort of the keys with iota values puts the C seeds first, by decreasing size and
//               ascending id: a seed's position is its cluster's number.  The count is where the seeds end.
//   grouping    labels = rank[name]; a second stable sort of the labels with iota values gives the member lists.
// Integer atomics only; the same input gives the same bits on every call.
//
// Density clustering (dbscan.hip; include/pcgx.h, "density clusters") comes through clusters_enqueue too: with min_pts
// >= 2 a count pass writes core flags where the usable flags would lie, the component passes run on them unchanged, a
// border pass stores every attached border point's core neighbour into its own parent word before the last pointer
// jumping, and the tail counts core and border points alike.
#include <math.h>
#include <stdlib.h>

#include "cluster_terms.h"
#include "dbscan.h"
#include "knn_grid.h"
#include "radius_graph.h"

namespace pcgx {

// the cut between two usable points
struct ClusterCut {
  float min_cos;
  int32_t oriented;
};

__device__ __forceinline__ uint32_t cl_id_at(const float4 *__restrict__ pts, const int64_t f) {
  return pts ? __float_as_uint(pts[f].w) : (uint32_t)f;
}

__global__ __launch_bounds__(256) void cl_init_kernel(uint32_t *__restrict__ parent, uint32_t *__restrict__ count,
                                                      uint32_t *__restrict__ min_id, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  parent[i] = (uint32_t)i;
  count[i] = 0u;
  min_id[i] = 0xffffffffu;
}

// ------------------------------------------------------------------ staging
__device__ __forceinline__ void cl_stage(const float x, const float y, const float z, const uint32_t id, const int64_t pos,
                                         const float bound, const float *__restrict__ normals,
                                         const float *__restrict__ curvature, const float max_curvature,
                                         uint8_t *__restrict__ usable, float4 *__restrict__ nrm) {
  const bool own = ref_dist_sq(x, y, z, x, y, z) < bound;  // i in N(i): false for a NaN or infinite coordinate
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (normals) {
    nx = normals[3 * (size_t)id];
    ny = normals[3 * (size_t)id + 1];
    nz = normals[3 * (size_t)id + 2];
  }
  const bool u = cluster_usable(own, normals != nullptr, nx, ny, nz, curvature != nullptr,
                                curvature ? curvature[id] : 0.0f, max_curvature);
  usable[pos] = u ? (uint8_t)1 : (uint8_t)0;
  if (nrm) nrm[pos] = make_float4(nx, ny, nz, u ? 1.0f : 0.0f);
}

// the record at every position of the grid's cell order
__global__ __launch_bounds__(256) void cl_stage_grid_kernel(GridView g, int64_t n, float bound,
                                                            const float *__restrict__ normals,
                                                            const float *__restrict__ curvature, float max_curvature,
                                                            uint8_t *__restrict__ usable, float4 *__restrict__ nrm) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  const float4 p = g.pts[f];
  cl_stage(p.x, p.y, p.z, __float_as_uint(p.w), f, bound, normals, curvature, max_curvature, usable, nrm);
}

// the record of every node of the tree, by id (the flags were zeroed: an id without a node, a deleted one, stays unusable)
__global__ __launch_bounds__(256) void cl_stage_tree_kernel(TreeView tv, float bound, const float *__restrict__ normals,
                                                            const float *__restrict__ curvature, float max_curvature,
                                                            uint8_t *__restrict__ usable, float4 *__restrict__ nrm) {
  float4 nd;
  if (!tree_slot_node(tv, blockIdx.x * 256u + threadIdx.x + 1u, &nd)) return;
  const uint32_t id = __float_as_uint(nd.w);
  cl_stage(nd.x, nd.y, nd.z, id, (int64_t)id, bound, normals, curvature, max_curvature, usable, nrm);
}

// ------------------------------------------------------------------ components
// What the edge test reads of a neighbour: nothing (a handle with a grid holds finite points only, so with neither normals
// nor curvature every point is usable), its usable flag, or its {nx, ny, nz, usable} record.
enum ClusterRead { kCutNone = 0, kCutFlags = 1, kCutNormals = 2 };

// The edge of the radius graph's passes (radius_graph.h): both ends usable, and with normals the cut.  flags: the byte at
// every position that says whether the point there takes part (density clustering passes its core flags).
template <int kCut>
struct ClusterEdge {
  static constexpr bool kWalks = kCut != kCutNone;
  const uint8_t *__restrict__ flags;
  const float4 *__restrict__ nrm;
  ClusterCut cut;
  __device__ __forceinline__ bool live(const uint32_t pos, uint32_t) const { return kCut == kCutNone || flags[pos] != 0; }
  __device__ __forceinline__ float4 mine(const uint32_t pos, uint32_t) const {
    if constexpr (kCut == kCutNormals) return nrm[pos];
    return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  // Does the staged record at position f join a usable point with the normal `mine`?
  __device__ __forceinline__ bool joins(const uint32_t f, uint32_t, const float4 &mine) const {
    if constexpr (kCut == kCutNormals) {
      const float4 s = nrm[f];
      return s.w != 0.0f && cluster_normals_agree(mine.x, mine.y, mine.z, s.x, s.y, s.z, cut.min_cos, cut.oriented);
    } else if constexpr (kCut == kCutFlags) {
      return flags[f] != 0;
    } else {
      return true;
    }
  }
};

// ------------------------------------------------------------------ sizes and names
// count[root] = usable points under it, min_id[root] = their smallest id.  The lanes of a wave are neighbours in space
// and mostly of one component: one atomic pair per distinct root of the wave (wave_root_flush, radius_graph.h, with the
// measured reason).  pts: the grid's records (positions -> ids), nullptr: positions are ids.
// Even so a cloud that is one component sends every wave's atomics to one word (218 us at 1M points), so the waves of a
// workgroup first put the first root each of them meets -- in cell order nearly always the only one -- into LDS, and the
// first wave merges those entries by the same method: a sixteenth of the atomics.  A wave's further roots go straight
// to memory.
constexpr int kStatsBlock = 1024, kStatsWaves = kStatsBlock / 64;

__global__ __launch_bounds__(kStatsBlock) void cl_root_stats_kernel(const float4 *__restrict__ pts, int64_t n,
                                                                    const uint32_t *__restrict__ parent,
                                                                    const uint8_t *__restrict__ usable,
                                                                    uint32_t *__restrict__ count, uint32_t *__restrict__ min_id) {
  __shared__ uint32_t s_root[kStatsWaves], s_cnt[kStatsWaves], s_min[kStatsWaves];
  const int64_t f = (int64_t)blockIdx.x * kStatsBlock + threadIdx.x;
  const bool valid = f < n && usable[f] != 0;
  const uint32_t root = valid ? parent[f] : 0xffffffffu;
  const uint32_t id = valid ? cl_id_at(pts, f) : 0xffffffffu;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long todo = __ballot(valid);
  uint32_t r0 = 0xffffffffu, c0 = 0u, m0 = 0xffffffffu;  // the wave's first root, its lanes and their smallest id
  if (todo) {  // uniform
    const int leader = __ffsll((long long)todo) - 1;
    r0 = (uint32_t)__builtin_amdgcn_readlane((int)root, leader);
    const bool mine = valid && root == r0;
    const unsigned long long same = __ballot(mine);
    m0 = mine ? id : 0xffffffffu;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t v = (uint32_t)__shfl_xor((int)m0, o);
      m0 = v < m0 ? v : m0;
    }
    c0 = (uint32_t)__popcll(same);
    todo &= ~same;
  }
  if (lane == 0) {
    s_root[wave] = r0;
    s_cnt[wave] = c0;
    s_min[wave] = m0;
  }
  wave_root_flush<true>(valid, root, 1u, id, lane, todo, count, min_id);  // the wave's other roots
  __syncthreads();
  if (wave == 0) {
    const bool v = lane < kStatsWaves && s_cnt[lane < kStatsWaves ? lane : 0] != 0u;
    const uint32_t rr = v ? s_root[lane] : 0xffffffffu, cc = v ? s_cnt[lane] : 0u, mm = v ? s_min[lane] : 0xffffffffu;
    wave_root_flush<true>(v, rr, cc, mm, lane, __ballot(v), count, min_id);
  }
}

// by id: the component's name (its smallest id; all ones for an unusable point), its size, and the point's sort key
__global__ __launch_bounds__(256) void cl_name_kernel(const float4 *__restrict__ pts, int64_t n,
                                                      const uint32_t *__restrict__ parent, const uint8_t *__restrict__ usable,
                                                      const uint32_t *__restrict__ count, const uint32_t *__restrict__ min_id,
                                                      int64_t min_size, int64_t max_size, uint32_t *__restrict__ name,
                                                      uint32_t *__restrict__ psize, uint32_t *__restrict__ key) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  const uint32_t id = cl_id_at(pts, f);
  uint32_t nm = 0xffffffffu, sz = 0u;
  if (usable[f]) {
    const uint32_t r = parent[f];
    nm = min_id[r];
    sz = count[r];
  }
  name[id] = nm;
  psize[id] = sz;
  key[id] = cluster_seed_key(nm == id, sz, (uint32_t)n, min_size, max_size);
}

// ------------------------------------------------------------------ ranking and grouping
// the sorted keys: seeds first.  rank[seed id] = its position; sizes; the count = where the seeds end
__global__ __launch_bounds__(256) void cl_rank_kernel(const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval,
                                                      int64_t n, uint32_t *__restrict__ rank, int32_t *__restrict__ sizes,
                                                      int32_t *__restrict__ n_clusters) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const uint32_t key = skey[k];
  const bool seed = key != (uint32_t)n;
  if (seed) rank[sval[k]] = (uint32_t)k;
  if (sizes) sizes[k] = seed ? (int32_t)cluster_key_size(key, (uint32_t)n) : 0;
  if (seed && (k + 1 == n || skey[k + 1] == (uint32_t)n)) *n_clusters = (int32_t)(k + 1);
  if (k == 0 && !seed) *n_clusters = 0;
}

__global__ __launch_bounds__(256) void cl_label_kernel(const uint32_t *__restrict__ name, const uint32_t *__restrict__ psize,
                                                       const uint32_t *__restrict__ rank, int64_t n, int64_t min_size,
                                                       int64_t max_size, int32_t *__restrict__ labels,
                                                       uint32_t *__restrict__ key2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t nm = name[i];
  const bool kept = nm != 0xffffffffu && cluster_size_kept(psize[i], min_size, max_size);
  const uint32_t lab = kept ? rank[nm] : (uint32_t)n;
  labels[i] = kept ? (int32_t)lab : -1;
  if (key2) key2[i] = lab;
}

// the ids sorted by label: the members of cluster 0 ascending, then those of cluster 1, ...; -1 where no cluster is left
__global__ __launch_bounds__(256) void cl_ids_kernel(const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval,
                                                     int64_t n, int32_t *__restrict__ ids) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) ids[k] = skey[k] != (uint32_t)n ? (int32_t)sval[k] : -1;
}

static int cl_key_bits(int64_t n) {  // keys are 0 .. n
  int b = 0;
  while (((int64_t)1 << b) <= n) b++;
  return b;
}

// (dbscan.h says what the arguments are)
pcgx_status clusters_enqueue(const pcgx_kdtree *a, int64_t n, float radius, const float *d_normals, float min_cos,
                             int32_t oriented, const float *d_curvature, float max_curvature, int64_t min_size,
                             int64_t max_size, const ClusterDensity *density, int32_t *d_labels, int32_t *d_n_clusters,
                             int32_t *d_sizes, int32_t *d_ids, hipStream_t st) {
  Arena &ar = ctx().arena;
  const unsigned nb = (unsigned)((n + 255) / 256);
  const float bound = radius * radius;
  const ClusterCut cut{min_cos, oriented};
  uint32_t *parent = nullptr, *count = nullptr, *min_id = nullptr, *name = nullptr, *psize = nullptr;
  uint32_t *keys[2] = {nullptr, nullptr}, *vals[2] = {nullptr, nullptr};
  uint8_t *usable = nullptr, *core = nullptr;
  float4 *nrm = nullptr;
  // dense: the edges join core points (core[]), and usable[] holds what the tail counts: 2 core, 1 attached border
  const bool dense = density && density->min_pts > 1;
  void *ws = nullptr;
  PCGX_TRY(ar.alloc_n((size_t)n, &parent));
  PCGX_TRY(ar.alloc_n((size_t)n, &count));
  PCGX_TRY(ar.alloc_n((size_t)n, &min_id));
  PCGX_TRY(ar.alloc_n((size_t)n, &name));
  PCGX_TRY(ar.alloc_n((size_t)n, &psize));
  for (int k = 0; k < 2; k++) {
    PCGX_TRY(ar.alloc_n((size_t)n, &keys[k]));
    PCGX_TRY(ar.alloc_n((size_t)n, &vals[k]));
  }
  PCGX_TRY(ar.alloc(radix_sort_workspace_bytes(n), &ws));
  if (d_normals) PCGX_TRY(ar.alloc_n((size_t)n, &nrm));
  PCGX_TRY(ar.alloc_n((size_t)n, &usable));
  if (dense) PCGX_TRY(ar.alloc_n((size_t)n, &core));

  hipLaunchKernelGGL(cl_init_kernel, dim3(nb), dim3(256), 0, st, parent, count, min_id, n);
  const bool on_grid = a && a->grid_ok && a->n == n && !range_walk_forced();  // (as region growing takes its source)
  const float4 *pts = on_grid ? a->grid.pts : nullptr;
  if (!on_grid) {
    PCGX_HIP_TRY(hipMemsetAsync(usable, 0, (size_t)n, st));
    if (dense) PCGX_HIP_TRY(hipMemsetAsync(core, 0, (size_t)n, st));
  }
  if (a) {
    if (dense) {
      dbscan_flags_launch(a, on_grid, n, bound, density->min_pts, density->count_all, core, st);
    } else if (on_grid) {
      hipLaunchKernelGGL(cl_stage_grid_kernel, dim3(nb), dim3(256), 0, st, a->grid, n, bound, d_normals, d_curvature,
                         max_curvature, usable, nrm);
    } else {
      const TreeView tv = a->view();
      hipLaunchKernelGGL(cl_stage_tree_kernel, dim3(((1u << tv.depth) + 255u) / 256u), dim3(256), 0, st, tv, bound,
                         d_normals, d_curvature, max_curvature, usable, nrm);
    }
    const uint8_t *flags = dense ? core : usable;  // the byte the edge test reads of a point
    if (d_normals)
      PCGX_TRY(rgraph_components_enqueue(a, on_grid, n, bound, ClusterEdge<kCutNormals>{flags, nrm, cut}, parent, st));
    else if (d_curvature || dense || !on_grid)
      PCGX_TRY(rgraph_components_enqueue(a, on_grid, n, bound, ClusterEdge<kCutFlags>{flags, nrm, cut}, parent, st));
    else
      PCGX_TRY(rgraph_components_enqueue(a, on_grid, n, bound, ClusterEdge<kCutNone>{flags, nrm, cut}, parent, st));
    if (dense) dbscan_border_launch(a, on_grid, n, bound, core, usable, parent, st);
    hipLaunchKernelGGL(uf_jump_kernel, dim3(nb), dim3(256), 0, st, parent, n);
  }
  hipLaunchKernelGGL(cl_root_stats_kernel, dim3((unsigned)((n + kStatsBlock - 1) / kStatsBlock)), dim3(kStatsBlock), 0, st,
                     pts, n, (const uint32_t *)parent,
                     (const uint8_t *)usable, count, min_id);
  hipLaunchKernelGGL(cl_name_kernel, dim3(nb), dim3(256), 0, st, pts, n, (const uint32_t *)parent, (const uint8_t *)usable,
                     (const uint32_t *)count, (const uint32_t *)min_id, min_size, max_size, name, psize, keys[0]);
  PCGX_HIP_TRY(hipGetLastError());
  const int bits = cl_key_bits(n);
  int r1 = 0;
  PCGX_TRY(radix_sort_pairs(keys, vals, n, bits, ws, &r1, st, true));
  uint32_t *rank = parent;  // (the union-find is done with)
  hipLaunchKernelGGL(cl_rank_kernel, dim3(nb), dim3(256), 0, st, (const uint32_t *)keys[r1], (const uint32_t *)vals[r1], n,
                     rank, d_sizes, d_n_clusters);
  hipLaunchKernelGGL(cl_label_kernel, dim3(nb), dim3(256), 0, st, (const uint32_t *)name, (const uint32_t *)psize,
                     (const uint32_t *)rank, n, min_size, max_size, d_labels, d_ids ? keys[0] : nullptr);
  PCGX_HIP_TRY(hipGetLastError());
  if (density && density->d_kind) dbscan_kind_launch(pts, n, usable, !dense, density->d_kind, st);
  if (d_ids) {
    int r2 = 0;
    PCGX_TRY(radix_sort_pairs(keys, vals, n, bits, ws, &r2, st, true));
    hipLaunchKernelGGL(cl_ids_kernel, dim3(nb), dim3(256), 0, st, (const uint32_t *)keys[r2], (const uint32_t *)vals[r2], n,
                       d_ids);
    PCGX_HIP_TRY(hipGetLastError());
  }
  return PCGX_OK;
}

constexpr int64_t kClusterMaxPoints = 0x7fffffff;  // ids are int32 on the device

pcgx_status clusters_check(const char *fn, const pcgx_kdtree *t, float radius, const void *normals, float min_cos,
                           const void *curvature, float max_curvature, int64_t min_size, int64_t max_size,
                           const void *labels, const void *n_clusters) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!(radius > 0.0f && radius < __builtin_inff())) return fail(PCGX_E_INVALID, "%s: radius must be finite and > 0", fn);
  if (normals && min_cos != min_cos) return fail(PCGX_E_INVALID, "%s: min_cos is NaN", fn);
  if (curvature && max_curvature != max_curvature) return fail(PCGX_E_INVALID, "%s: max_curvature is NaN", fn);
  if (min_size < 0 || max_size < 0) return fail(PCGX_E_INVALID, "%s: min_size and max_size must be >= 0", fn);
  if (max_size > 0 && max_size < (min_size > 1 ? min_size : 1))
    return fail(PCGX_E_INVALID, "%s: max_size is below max(min_size, 1)", fn);
  if (t->n > kClusterMaxPoints) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points", fn);
  if (t->n > 0 && (!labels || !n_clusters)) return fail(PCGX_E_INVALID, "%s: NULL labels or n_clusters", fn);
  return PCGX_OK;
}

}  // namespace pcgx

using namespace pcgx;

extern "C" pcgx_status pcgx_kdtree_clusters_dev(const pcgx_kdtree *t, float radius, const float *d_normals, float min_cos,
                                                int32_t oriented, const float *d_curvature, float max_curvature,
                                                int64_t min_size, int64_t max_size, int32_t *d_labels,
                                                int32_t *d_n_clusters, int32_t *d_sizes, int32_t *d_ids, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(clusters_check("pcgx_kdtree_clusters_dev", t, radius, d_normals, min_cos, d_curvature, max_curvature, min_size,
                          max_size, d_labels, d_n_clusters));
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
  return clusters_enqueue(empty ? nullptr : a, n, radius, d_normals, min_cos, oriented, d_curvature, max_curvature, min_size,
                          max_size, nullptr, d_labels, d_n_clusters, d_sizes, d_ids, st);
}

extern "C" pcgx_status pcgx_kdtree_clusters(const pcgx_kdtree *t, float radius, const float *normals, float min_cos,
                                            int32_t oriented, const float *curvature, float max_curvature, int64_t min_size,
                                            int64_t max_size, int64_t *labels, int64_t *n_clusters, int64_t *sizes,
                                            int64_t *ids) {
  PCGX_API_CALL();
  PCGX_TRY(clusters_check("pcgx_kdtree_clusters", t, radius, normals, min_cos, curvature, max_curvature, min_size, max_size,
                          labels, n_clusters));
  const int64_t n = t->n;
  if (n == 0) {
    if (n_clusters) *n_clusters = 0;
    return PCGX_OK;
  }
  PCGX_TRY(ensure_init());
  // always on the device: the components, the ranking and the grouping are the kernels', not a host restatement
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_nrm = nullptr, *d_curv = nullptr;
  int32_t *d_out = nullptr;  // labels [n], sizes [n], ids [n], the count
  if (normals) {
    PCGX_TRY(ha.alloc_n((size_t)n * 3, &d_nrm));
    PCGX_TRY(staged_upload(d_nrm, normals, (size_t)n * 12, st));
  }
  if (curvature) {
    PCGX_TRY(ha.alloc_n((size_t)n, &d_curv));
    PCGX_TRY(staged_upload(d_curv, curvature, (size_t)n * 4, st));
  }
  PCGX_TRY(ha.alloc_n((size_t)n * 3 + 1, &d_out));
  PCGX_TRY(pcgx_kdtree_clusters_dev(t, radius, d_nrm, min_cos, oriented, d_curv, max_curvature, min_size, max_size, d_out,
                                    d_out + 3 * n, sizes ? d_out + n : nullptr, ids ? d_out + 2 * n : nullptr, st));
  RawVector<int32_t> h((size_t)n * 3 + 1);
  PCGX_TRY(staged_download(h.data(), d_out, ((size_t)n * 3 + 1) * 4, st));
  for (int64_t i = 0; i < n; i++) labels[i] = h[(size_t)i];
  if (sizes)
    for (int64_t i = 0; i < n; i++) sizes[i] = h[(size_t)(n + i)];
  if (ids)
    for (int64_t i = 0; i < n; i++) ids[i] = h[(size_t)(2 * n + i)];
  *n_clusters = h[(size_t)(3 * n)];
  return PCGX_OK;
}
