// keypoints.hip -- local maxima of a per-point score over radius neighbourhoods, and ISS keypoints (Zhong 2009) made
// from them (extension: no reference parity; include/pcgx.h, "keypoints").
//
// What stands between the FPFH chain and a large cloud: the matcher is brute force over all pairs, so it is run over a
// few thousand keypoints instead of every point.  Both operations work over a tree's own points, as query_source lays
// them out, on each of the three kinds of handle (grid, forced walk, patched tree after DeletePoint):
//   eigenvalue stage (ISS)  normals_kernel itself (normals.hip): its moments and its Jacobi solve, the eigenvalues and the
//                           saliency two more outputs of normals_finish.
//   local_maxima_kernel     a fourth consumer of the shared enumeration (radius_visit.h), one query per lane.  Per record
//                           inside the bound: its score by id (4 bytes), and two bits -- "beaten" (keypoint_terms.h) and
//                           "met myself" (a deleted id or a NaN coordinate never meets itself: no flags array needed).
//                           A lane whose own score cannot qualify enumerates nothing.  One flag byte per id.
//   compaction              the flags to ascending ids by bucket_grid.h's tile compaction (count, scan, write), then the
//                           -1 tail.  The scan leaves the total in the caller's count word.
// Of a fat row's shares the two bits are combined over the wave by ballots, and the owner merges them.
#include <math.h>
#include <stdlib.h>

#include "bucket_grid.h"
#include "keypoint_terms.h"
#include "radius_visit.h"

namespace pcgx {

// normals.hip
pcgx_status normals_iss_enqueue(const pcgx_kdtree *t, float radius, int32_t min_neighbors, float gamma_21, float gamma_32,
                                float *d_eigenvalues, float *d_saliency, hipStream_t st);

constexpr int kKeyBlock = kRangeWalkBlock;  // one wave per workgroup: the walks' LDS frame stacks are [level][64]

// the two bits of one query
struct MaxBits {
  bool beaten, met;

  // the record p, inside the bound of query i (score si)
  __device__ __forceinline__ void take(const float *__restrict__ score, const float4 &p, const float si, const int32_t i) {
    const int32_t j = (int32_t)__float_as_uint(p.w);
    met = met || j == i;
    if (!beaten) beaten = keypoint_beats(score[j], j, si, i);
  }
};

template <int kSrc>
__global__ __launch_bounds__(kKeyBlock) void local_maxima_kernel(GridView g, TreeView tv, XTreeView xv, QuerySource Q,
                                                                 float bound, const float *__restrict__ score,
                                                                 uint8_t *__restrict__ flag, int64_t guard) {
  extern __shared__ uint32_t s_stack[];
  const uint32_t n_tiles = (uint32_t)((Q.nq + kKeyBlock - 1) / kKeyBlock);
  const int64_t pos = (int64_t)xcd_tile(blockIdx.x, n_tiles) * kKeyBlock + threadIdx.x;
  const bool live = pos < Q.nq;
  int64_t i64 = 0;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f, si = 0.0f;
  if (live) {
    read_query(Q, pos, i64, qx, qy, qz);
    si = score[i64];
  }
  const int32_t i = (int32_t)i64;
  const bool cand = live && keypoint_candidate(si);  // nothing to enumerate for a score that cannot qualify
  MaxBits b{false, false};
  const int lane = (int)(threadIdx.x & 63u);
  radius_visit<kSrc>(
      RadiusViews{g, tv, xv, guard}, s_stack + threadIdx.x, kKeyBlock, qx, qy, qz, bound, cand,
      [&](const float4 &p, float) { b.take(score, p, si, i); },
      [&](int owner, float, float, float, auto rows) {  // the two bits, combined over the wave by ballots
        const float osi = __shfl(si, owner);
        const int32_t oi = __shfl(i, owner);
        MaxBits part{false, false};
        rows([&](const float4 &p, float) { part.take(score, p, osi, oi); });
        const bool any_beaten = __ballot(part.beaten) != 0ull, any_met = __ballot(part.met) != 0ull;
        if (lane == owner) {
          b.beaten = b.beaten || any_beaten;
          b.met = b.met || any_met;
        }
      });
  if (!live) return;
  flag[i64] = (cand && b.met && !b.beaten) ? (uint8_t)1 : (uint8_t)0;
}

__global__ __launch_bounds__(256) void keypoints_count_kernel(const uint8_t *__restrict__ flag, int64_t n,
                                                              uint32_t *__restrict__ tile_count) {
  tile_flag_count(n, [&](int64_t j) { return flag[j] != 0; }, tile_count);
}
__global__ __launch_bounds__(1024) void keypoints_scan_kernel(uint32_t *__restrict__ tile_count, int ntiles,
                                                              uint32_t *__restrict__ total) {
  tile_scan(tile_count, ntiles, total);
}
__global__ __launch_bounds__(256) void keypoints_write_kernel(const uint8_t *__restrict__ flag, int64_t n,
                                                              const uint32_t *__restrict__ tile_offset,
                                                              int32_t *__restrict__ ids) {
  tile_flag_write(n, [&](int64_t j) { return flag[j] != 0; }, tile_offset,
                  [=](uint32_t slot, int64_t j) { ids[slot] = (int32_t)j; });
}
// the slots from the count on: -1 (the write kernel fills [0, count): the two touch different slots)
__global__ __launch_bounds__(256) void keypoints_tail_kernel(const int32_t *__restrict__ n_ids, int64_t n,
                                                             int32_t *__restrict__ ids) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n && j >= (int64_t)*n_ids) ids[j] = -1;
}

// One flag byte per id -> the flagged ids in ascending order, -1 in every remaining slot, their number in *d_n_ids.
// tile_count: ceil(n / kRunTile) words of the caller's.  boundary.hip compacts its flags through this too.
pcgx_status flags_to_ids_enqueue(const uint8_t *d_flag, int64_t n, uint32_t *tile_count, int32_t *d_ids, int32_t *d_n_ids,
                                 hipStream_t st) {
  const int ntiles = (int)((n + kRunTile - 1) / kRunTile);
  hipLaunchKernelGGL(keypoints_count_kernel, dim3(ntiles), dim3(256), 0, st, d_flag, n, tile_count);
  hipLaunchKernelGGL(keypoints_scan_kernel, dim3(1), dim3(1024), 0, st, tile_count, ntiles, (uint32_t *)d_n_ids);
  hipLaunchKernelGGL(keypoints_write_kernel, dim3(ntiles), dim3(256), 0, st, d_flag, n, (const uint32_t *)tile_count, d_ids);
  hipLaunchKernelGGL(keypoints_tail_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const int32_t *)d_n_ids, n,
                     d_ids);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

template <int kSrc>
void maxima_launch(const pcgx_kdtree *t, const TreeView &tv, const XTreeView &xv, const QuerySource &Q, float bound,
                   const float *d_score, uint8_t *d_flag, size_t stack_bytes, hipStream_t st) {
  const dim3 grid(xcd_grid((unsigned)((Q.nq + kKeyBlock - 1) / kKeyBlock))), block(kKeyBlock);
  const GridView g = kSrc == kRangeGrid ? t->grid : GridView{};
  hipLaunchKernelGGL(local_maxima_kernel<kSrc>, grid, block, stack_bytes, st, g, tv, xv, Q, bound, d_score, d_flag,
                     xwalk_guard(t->n));
}

// Len() > 0, everything device resident; temporaries from ctx().arena, which the caller has begun
pcgx_status maxima_enqueue(const pcgx_kdtree *t, float radius, const float *d_score, int32_t *d_ids, int32_t *d_n_ids,
                           hipStream_t st) {
  const int64_t n = t->n;
  const RangeSrc src = range_source(t);  // as pcgx_kdtree_range_count takes it
  XTreeView xv{};
  if (src == kRangeXWalk) PCGX_TRY(xtree_view(t, &xv, st));
  const TreeView tv = t->view();
  QuerySource Q;
  PCGX_TRY(query_source(t, src, nullptr, n, &Q, st));
  const int ntiles = (int)((n + kRunTile - 1) / kRunTile);
  uint8_t *d_flag = nullptr;
  uint32_t *tile_count = nullptr;
  PCGX_TRY(ctx().arena.alloc_n((size_t)n, &d_flag));
  PCGX_TRY(ctx().arena.alloc_n((size_t)ntiles, &tile_count));
  const float bound = radius * radius;
  if (src == kRangeXWalk) maxima_launch<kRangeXWalk>(t, tv, xv, Q, bound, d_score, d_flag, xwalk_stack_bytes(xv, kKeyBlock), st);
  else if (src == kRangeGrid) maxima_launch<kRangeGrid>(t, tv, xv, Q, bound, d_score, d_flag, 0, st);
  else maxima_launch<kRangeWalk>(t, tv, xv, Q, bound, d_score, d_flag, walk_stack_bytes(tv, kKeyBlock), st);
  return flags_to_ids_enqueue(d_flag, n, tile_count, d_ids, d_n_ids, st);
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kKeyMaxPoints = 0x7fffffff;  // ids are int32 on the device

bool finite_positive(float v) { return v > 0.0f && v < __builtin_inff(); }

pcgx_status maxima_check(const char *fn, const pcgx_kdtree *t, float radius, const void *score, const void *ids,
                         const void *n_ids) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!finite_positive(radius)) return fail(PCGX_E_INVALID, "%s: radius must be finite and > 0", fn);
  if (t->n > kKeyMaxPoints) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points", fn);
  if (t->n > 0 && (!score || !ids || !n_ids)) return fail(PCGX_E_INVALID, "%s: NULL score, ids or n_ids", fn);
  return PCGX_OK;
}

pcgx_status iss_check(const char *fn, const pcgx_kdtree *t, float salient_radius, float non_max_radius, float gamma_21,
                      float gamma_32, const void *ids, const void *n_ids) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!finite_positive(salient_radius) || !finite_positive(non_max_radius))
    return fail(PCGX_E_INVALID, "%s: both radii must be finite and > 0", fn);
  if (!finite_positive(gamma_21) || !finite_positive(gamma_32))
    return fail(PCGX_E_INVALID, "%s: both gammas must be finite and > 0", fn);
  if (t->n > kKeyMaxPoints) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points", fn);
  if (t->n > 0 && (!ids || !n_ids)) return fail(PCGX_E_INVALID, "%s: NULL ids or n_ids", fn);
  return PCGX_OK;
}

// ids [n] and the count behind them, from the device to the host's int64
pcgx_status ids_to_host(const int32_t *d_out, int64_t n, int64_t *ids, int64_t *n_ids, hipStream_t st) {
  RawVector<int32_t> h((size_t)n + 1);
  PCGX_TRY(staged_download(h.data(), d_out, ((size_t)n + 1) * 4, st));
  for (int64_t i = 0; i < n; i++) ids[i] = h[(size_t)i];
  *n_ids = h[(size_t)n];
  return PCGX_OK;
}

}  // namespace

extern "C" pcgx_status pcgx_kdtree_local_maxima_dev(const pcgx_kdtree *t, float radius, const float *d_score,
                                                    int32_t *d_ids, int32_t *d_n_ids, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(maxima_check("pcgx_kdtree_local_maxima_dev", t, radius, d_score, d_ids, d_n_ids));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  if (t->n == 0) {
    if (d_n_ids) PCGX_HIP_TRY(hipMemsetAsync(d_n_ids, 0, sizeof(int32_t), st));
    return PCGX_OK;
  }
  PCGX_TRY(ctx().arena.begin(st));
  return maxima_enqueue(t, radius, d_score, d_ids, d_n_ids, st);
}

extern "C" pcgx_status pcgx_kdtree_local_maxima(const pcgx_kdtree *t, float radius, const float *score, int64_t *ids,
                                                int64_t *n_ids) {
  PCGX_API_CALL();
  PCGX_TRY(maxima_check("pcgx_kdtree_local_maxima", t, radius, score, ids, n_ids));
  const int64_t n = t->n;
  if (n == 0) {
    if (n_ids) *n_ids = 0;
    return PCGX_OK;
  }
  PCGX_TRY(ensure_init());
  // always on the device: the enumeration and the compaction are the kernels', not a host restatement
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_s = nullptr;
  int32_t *d_out = nullptr;  // ids [n], the count
  PCGX_TRY(ha.alloc_n((size_t)n, &d_s));
  PCGX_TRY(staged_upload(d_s, score, (size_t)n * 4, st));
  PCGX_TRY(ha.alloc_n((size_t)n + 1, &d_out));
  PCGX_TRY(pcgx_kdtree_local_maxima_dev(t, radius, d_s, d_out, d_out + n, st));
  return ids_to_host(d_out, n, ids, n_ids, st);
}

extern "C" pcgx_status pcgx_kdtree_iss_keypoints_dev(const pcgx_kdtree *t, float salient_radius, float non_max_radius,
                                                     float gamma_21, float gamma_32, int32_t min_neighbors,
                                                     float *d_eigenvalues, float *d_saliency, int32_t *d_ids,
                                                     int32_t *d_n_ids, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(iss_check("pcgx_kdtree_iss_keypoints_dev", t, salient_radius, non_max_radius, gamma_21, gamma_32, d_ids, d_n_ids));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  if (t->n == 0) {
    if (d_n_ids) PCGX_HIP_TRY(hipMemsetAsync(d_n_ids, 0, sizeof(int32_t), st));
    return PCGX_OK;
  }
  PCGX_TRY(ctx().arena.begin(st));
  if (!d_saliency) PCGX_TRY(ctx().arena.alloc_n((size_t)t->n, &d_saliency));
  PCGX_TRY(normals_iss_enqueue(t, salient_radius, min_neighbors, gamma_21, gamma_32, d_eigenvalues, d_saliency, st));
  return maxima_enqueue(t, non_max_radius, d_saliency, d_ids, d_n_ids, st);
}

extern "C" pcgx_status pcgx_kdtree_iss_keypoints(const pcgx_kdtree *t, float salient_radius, float non_max_radius,
                                                 float gamma_21, float gamma_32, int32_t min_neighbors,
                                                 float *eigenvalues, float *saliency, int64_t *ids, int64_t *n_ids) {
  PCGX_API_CALL();
  PCGX_TRY(iss_check("pcgx_kdtree_iss_keypoints", t, salient_radius, non_max_radius, gamma_21, gamma_32, ids, n_ids));
  const int64_t n = t->n;
  if (n == 0) {
    if (n_ids) *n_ids = 0;
    return PCGX_OK;
  }
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_e = nullptr, *d_s = nullptr;
  int32_t *d_out = nullptr;  // ids [n], the count
  if (eigenvalues) PCGX_TRY(ha.alloc_n((size_t)n * 3, &d_e));
  if (saliency) PCGX_TRY(ha.alloc_n((size_t)n, &d_s));
  PCGX_TRY(ha.alloc_n((size_t)n + 1, &d_out));
  PCGX_TRY(pcgx_kdtree_iss_keypoints_dev(t, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, d_e, d_s,
                                         d_out, d_out + n, st));
  if (eigenvalues) PCGX_TRY(staged_download(eigenvalues, d_e, (size_t)n * 12, st));
  if (saliency) PCGX_TRY(staged_download(saliency, d_s, (size_t)n * 4, st));
  return ids_to_host(d_out, n, ids, n_ids, st);
}
