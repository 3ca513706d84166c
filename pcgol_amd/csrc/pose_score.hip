// pose_score.hip -- K poses scored against the whole clouds in one call, and the selection of the hypotheses worth
// scoring (extension: no reference parity; include/pcgx.h, "score poses").  For every pose: how many source points land
// within max_dist of the tree, and the float64 sum of their DistSq -- what pcgx_kdtree_nearest_batch would answer for
// the moved points, with nothing written per pair and nothing read back.  pose_score_plan.h decides the path, the chunk
// and every temporary's size; this file allocates and enqueues what it says.
//   score_key_kernel       the source's Morton keys over its own box (read from device memory: launch_minmax's output)
//   score_gather_kernel    the source in that order, {x, y, z, 0} records: a rigid motion keeps neighbouring lanes on
//                          neighbouring cells under every pose
//   score_fused_kernel     the hot one.  A lane owns a source point, a workgroup a tile of them and ONE pose
//                          (blockIdx.y): the pose's 16 numbers are workgroup-uniform and sit in scalar registers.  The
//                          lane transforms its point, asks grid_nearest (no hint) and keeps count and float64 sum in
//                          registers.  A GRID_WALK verdict (tie, DistSq == max_dist^2, a region wider than the grid
//                          certifies) puts x' into slot pose-in-chunk * n + position and the slot on the walk's list --
//                          one returning atomic per wave -- and a bit into the wave's mask word.  One {count, walks,
//                          sum} partial per workgroup: lanes by a fixed shuffle tree, waves in ascending order.
//   score_walk_add_kernel  behind the walk (knn.hip, launch_nearest_listed): the same tiles; a workgroup whose partial
//                          says "no walks" leaves at once, the others add the walk's answers of their masked lanes to
//                          their own partial.  No atomics on the sums anywhere: the bits are the same on every call.
//   score_transform_kernel, score_count_kernel
//                          the plain path (handles with deletions, walk-only handles): one pose's x' into a buffer, the
//                          handle's own search, then the tiles' partials from ids and DistSq.
//   score_reduce_kernel    one workgroup per pose: the tiles' partials in a fixed order -> counts[k], sums[k]
//   score_finish_kernel    ONE workgroup: the first best live pose and the result record, every word
//   pose_select_kernel     ONE workgroup: K rounds of a first-maximum search over the hypotheses' keys, each round below
//                          the last one's key (keys are distinct): no sort, no flags
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "knn_grid.h"
#include "pcgx_internal.h"
#include "pose_score_plan.h"

namespace pcgx {

constexpr int kScoreTile = 256;
constexpr int kScoreWaves = kScoreTile / 64;
constexpr int kScoreKeyBits = 5;  // per axis, as morton_order's
constexpr int kSelectBlock = 1024;
constexpr int kSelectWaves = kSelectBlock / 64;

struct ScorePartial {
  int32_t count;  // found pairs of the tile under the pose
  int32_t walks;  // pairs the grid left to the walk (their answers are added by score_walk_add_kernel)
  double sum;     // of the found pairs' DistSq
};
static_assert(sizeof(ScorePartial) == 16, "pose_score_plan.h: ScoreFacts::partial_rec");
static_assert(ScoreFacts().tile == kScoreTile && ScoreFacts().wave == 64, "pose_score_plan.h: ScoreFacts");

__device__ __forceinline__ bool score_finite3(float x, float y, float z) {
  const float inf = __builtin_inff();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;
}

// a pose whose 16 numbers all compare equal to 0 is dead (a NaN compares unequal: live)
__device__ __forceinline__ bool score_pose_live(const float *__restrict__ m) {
  bool live = false;
#pragma unroll
  for (int i = 0; i < 16; i++) live = live || !(m[i] == 0.0f);
  return live;
}

__device__ __forceinline__ uint32_t score_spread3(uint32_t v) {  // 5 bits -> every third bit
  return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6) | ((v & 16u) << 8);
}

__global__ __launch_bounds__(256) void score_key_kernel(const float *__restrict__ src, int64_t n,
                                                        const float *__restrict__ box6, uint32_t *__restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float cells = (float)(1u << kScoreKeyBits), cmax = cells - 1.0f;
  uint32_t c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float lo = box6[k], hi = box6[3 + k], ext = hi - lo;
    const float scale = (ext > 0.0f && ext < 3.0e38f) ? cells / ext : 0.0f;
    float f = (src[3 * i + k] - (lo == lo ? lo : 0.0f)) * scale;
    f = fminf(fmaxf(f, 0.0f), cmax);  // NaN -> 0: only the order depends on it
    c[k] = (uint32_t)f;
  }
  keys[i] = score_spread3(c[0]) | (score_spread3(c[1]) << 1) | (score_spread3(c[2]) << 2);
}

__global__ __launch_bounds__(256) void score_gather_kernel(const float *__restrict__ src, int64_t n,
                                                           const uint32_t *__restrict__ order,
                                                           float4 *__restrict__ src4) {
  const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pos >= n) return;
  const int64_t i = order ? (int64_t)order[pos] : pos;
  src4[pos] = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], 0.0f);
}

// the workgroup's {count, sum}: lanes by a fixed tree, waves in ascending order; valid in thread 0 (all threads must
// be here)
__device__ __forceinline__ void score_block_fold(int32_t &cnt, double &sum, int32_t *s_cnt, double *s_sum) {
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    cnt += __shfl_xor(cnt, x);
    sum += __shfl_xor(sum, x);
  }
  const int t = (int)threadIdx.x;
  if ((t & 63) == 0) {
    s_cnt[t >> 6] = cnt;
    s_sum[t >> 6] = sum;
  }
  __syncthreads();
  if (t == 0) {
    cnt = s_cnt[0];
    sum = s_sum[0];
#pragma unroll
    for (int w = 1; w < kScoreWaves; w++) {
      cnt += s_cnt[w];
      sum += s_sum[w];
    }
  }
}

__global__ __launch_bounds__(kScoreTile) void score_fused_kernel(GridView g, const float4 *__restrict__ src4, int32_t n,
                                                                 uint32_t ntiles, const float *__restrict__ poses,
                                                                 float max_range_sq,
                                                                 ScorePartial *__restrict__ partials,
                                                                 unsigned long long *__restrict__ masks,
                                                                 float *__restrict__ walk_q,
                                                                 int32_t *__restrict__ walk_list,
                                                                 uint32_t *__restrict__ walk_count) {
  __shared__ int32_t s_cnt[kScoreWaves];
  __shared__ double s_sum[kScoreWaves];
  const uint32_t tile = xcd_tile(blockIdx.x, ntiles);
  if (tile >= ntiles) return;  // (workgroup-uniform)
  const int t = (int)threadIdx.x, wave = t >> 6;
  const uint32_t kc = blockIdx.y;  // the pose, counted from the chunk's first (poses points at that one)
  const size_t group = (size_t)kc * ntiles + tile;
  const float *__restrict__ m = poses + 16 * (size_t)kc;  // (workgroup-uniform: scalar loads)
  if (!score_pose_live(m)) {
    if (t == 0) partials[group] = ScorePartial{0, 0, 0.0};
    if ((t & 63) == 0) masks[group * kScoreWaves + wave] = 0ull;
    return;
  }
  const int64_t pos = (int64_t)tile * kScoreTile + t;
  const bool in = pos < n;
  const float4 p = src4[in ? pos : (int64_t)n - 1];
  float x, y, z;
  mat4_transform(m, p.x, p.y, p.z, x, y, z);
  int32_t cnt = 0;
  double sum = 0.0;
  bool walk = false;
  if (in && score_finite3(x, y, z)) {
    float4 best;
    float best_d;
    const GridVerdict v = grid_nearest(g, x, y, z, max_range_sq, __builtin_inff(), best, best_d);
    if (v == GRID_FOUND) {
      cnt = 1;
      sum = (double)best_d;
    } else if (v == GRID_WALK) {
      walk = true;
    }
  }
  const unsigned long long mask = __ballot(walk);
  if (mask != 0ull) {  // (wave-uniform)
    uint32_t base = 0u;
    if ((t & 63) == 0) base = atomicAdd(walk_count, (uint32_t)__popcll(mask));
    base = (uint32_t)__shfl((int)base, 0);
    if (walk) {
      const int64_t slot = (int64_t)kc * n + pos;  // (< 2^31: the plan's chunk)
      walk_q[3 * slot] = x;
      walk_q[3 * slot + 1] = y;
      walk_q[3 * slot + 2] = z;
      const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << (t & 63)) - 1ull));
      walk_list[base + rank] = (int32_t)slot;
    }
  }
  if ((t & 63) == 0) masks[group * kScoreWaves + wave] = mask;
  __shared__ int32_t s_walks[kScoreWaves];
  if ((t & 63) == 0) s_walks[wave] = (int32_t)__popcll(mask);
  score_block_fold(cnt, sum, s_cnt, s_sum);  // (its barrier covers s_walks)
  if (t == 0) {
    int32_t w = 0;
#pragma unroll
    for (int k = 0; k < kScoreWaves; k++) w += s_walks[k];
    partials[group] = ScorePartial{cnt, w, sum};
  }
}

__global__ __launch_bounds__(kScoreTile) void score_walk_add_kernel(int32_t n, uint32_t ntiles,
                                                                    const unsigned long long *__restrict__ masks,
                                                                    const int32_t *__restrict__ walk_ids,
                                                                    const float *__restrict__ walk_dsq,
                                                                    ScorePartial *__restrict__ partials) {
  __shared__ int32_t s_cnt[kScoreWaves];
  __shared__ double s_sum[kScoreWaves];
  const uint32_t tile = blockIdx.x, kc = blockIdx.y;
  const size_t group = (size_t)kc * ntiles + tile;
  if (partials[group].walks == 0) return;  // (workgroup-uniform)
  const int t = (int)threadIdx.x;
  const unsigned long long mask = masks[group * kScoreWaves + (t >> 6)];
  int32_t cnt = 0;
  double sum = 0.0;
  if ((mask >> (t & 63)) & 1ull) {
    const int64_t slot = (int64_t)kc * n + (int64_t)tile * kScoreTile + t;
    if (walk_ids[slot] >= 0) {
      cnt = 1;
      sum = (double)walk_dsq[slot];
    }
  }
  score_block_fold(cnt, sum, s_cnt, s_sum);
  if (t == 0) {
    ScorePartial r = partials[group];
    r.count += cnt;
    r.sum += sum;  // the grid's part, then the walk's
    partials[group] = r;
  }
}

__global__ __launch_bounds__(256) void score_transform_kernel(const float *__restrict__ src, int64_t n,
                                                              const float *__restrict__ pose, float *__restrict__ q) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float nan = __builtin_nanf("");
  float x = nan, y = nan, z = nan;
  if (score_pose_live(pose)) mat4_transform(pose, src[3 * i], src[3 * i + 1], src[3 * i + 2], x, y, z);
  q[3 * i] = x;
  q[3 * i + 1] = y;
  q[3 * i + 2] = z;
}

__global__ __launch_bounds__(kScoreTile) void score_count_kernel(const float *__restrict__ q, int64_t n,
                                                                 const int32_t *__restrict__ ids,
                                                                 const float *__restrict__ dsq,
                                                                 ScorePartial *__restrict__ partials) {
  __shared__ int32_t s_cnt[kScoreWaves];
  __shared__ double s_sum[kScoreWaves];
  const int64_t i = (int64_t)blockIdx.x * kScoreTile + threadIdx.x;
  int32_t cnt = 0;
  double sum = 0.0;
  if (i < n && score_finite3(q[3 * i], q[3 * i + 1], q[3 * i + 2]) && ids[i] >= 0) {
    cnt = 1;
    sum = (double)dsq[i];
  }
  score_block_fold(cnt, sum, s_cnt, s_sum);
  if (threadIdx.x == 0) partials[blockIdx.x] = ScorePartial{cnt, 0, sum};
}

__global__ __launch_bounds__(kScoreTile) void score_reduce_kernel(const ScorePartial *__restrict__ partials,
                                                                  uint32_t ntiles, int32_t *__restrict__ counts,
                                                                  double *__restrict__ sums) {
  __shared__ int32_t s_cnt[kScoreWaves];
  __shared__ double s_sum[kScoreWaves];
  const uint32_t kc = blockIdx.x;
  int32_t cnt = 0;  // (<= n < 2^31)
  double sum = 0.0;
  for (uint32_t tile = threadIdx.x; tile < ntiles; tile += kScoreTile) {  // ascending
    const ScorePartial r = partials[(size_t)kc * ntiles + tile];
    cnt += r.count;
    sum += r.sum;
  }
  score_block_fold(cnt, sum, s_cnt, s_sum);
  if (threadIdx.x == 0) {
    counts[kc] = cnt;
    sums[kc] = sum;
  }
}

__global__ __launch_bounds__(kScoreTile) void score_finish_kernel(const float *__restrict__ poses, int32_t K, int32_t n,
                                                                  const int32_t *__restrict__ counts,
                                                                  const double *__restrict__ sums,
                                                                  int32_t *__restrict__ result) {
  __shared__ unsigned long long s_key[kScoreWaves];
  __shared__ int32_t s_live[kScoreWaves];
  const int t = (int)threadIdx.x;
  // the live pose with the largest count, the smallest k among equals; 0: no pose is live
  unsigned long long key = 0ull;
  int32_t live = 0;
  for (int64_t k = t; k < K; k += kScoreTile)
    if (score_pose_live(poses + 16 * k)) {
      live++;
      const unsigned long long c = ((unsigned long long)((uint32_t)counts[k] + 1u) << 32) | (~(uint32_t)k);
      key = c > key ? c : key;
    }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    const unsigned long long o = __shfl_xor(key, x);
    key = o > key ? o : key;
    live += __shfl_xor(live, x);
  }
  if ((t & 63) == 0) {
    s_key[t >> 6] = key;
    s_live[t >> 6] = live;
  }
  __syncthreads();
  key = 0ull;
  live = 0;
#pragma unroll
  for (int w = 0; w < kScoreWaves; w++) {
    key = s_key[w] > key ? s_key[w] : key;
    live += s_live[w];
  }
  const int32_t best = key ? (int32_t)(~(uint32_t)key) : -1;
  if (t == 0) {
    result[0] = best;
    result[1] = key ? (int32_t)((uint32_t)(key >> 32) - 1u) : 0;
    result[2] = live;
    result[3] = n;
    const double s = best >= 0 ? sums[best] : 0.0;
    memcpy(&result[4], &s, 8);
    result[6] = result[7] = 0;
  }
  if (t < 16) ((float *)result)[8 + t] = best >= 0 ? poses[16 * (int64_t)best + t] : 0.0f;
}

__global__ __launch_bounds__(kSelectBlock) void pose_select_kernel(const int32_t *__restrict__ status,
                                                                   const int32_t *__restrict__ counts,
                                                                   const float *__restrict__ poses, int32_t n_hyp,
                                                                   int32_t K, int32_t *__restrict__ ids,
                                                                   float *__restrict__ out_poses,
                                                                   int32_t *__restrict__ n_selected) {
  __shared__ unsigned long long s_key[kSelectWaves];
  const int t = (int)threadIdx.x;
  unsigned long long below = ~0ull;  // the last round's key: this round's lies below it
  int32_t j = 0;
  for (; j < K; j++) {  // (every variable of the loop's control is workgroup-uniform)
    unsigned long long key = 0ull;
    for (int32_t h = t; h < n_hyp; h += kSelectBlock) {
      const int32_t c = counts[h];
      if (status[h] == 0 && c >= 3) {
        const unsigned long long k = ((unsigned long long)(uint32_t)c << 32) | (~(uint32_t)h);
        key = (k < below && k > key) ? k : key;
      }
    }
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) {
      const unsigned long long o = __shfl_xor(key, x);
      key = o > key ? o : key;
    }
    if ((t & 63) == 0) s_key[t >> 6] = key;
    __syncthreads();
    key = 0ull;
#pragma unroll
    for (int w = 0; w < kSelectWaves; w++) key = s_key[w] > key ? s_key[w] : key;
    __syncthreads();
    if (key == 0ull) break;  // no hypothesis is left
    const int32_t h = (int32_t)(~(uint32_t)key);
    if (t == 0) ids[j] = h;
    if (t < 16) out_poses[16 * (int64_t)j + t] = poses[16 * (int64_t)h + t];
    below = key;
  }
  if (t == 0) *n_selected = j;
  for (int64_t s = (int64_t)j + (t >> 4); s < K; s += kSelectBlock / 16) {  // the slots behind the last one
    if ((t & 15) == 0) ids[s] = -1;
    out_poses[16 * s + (t & 15)] = 0.0f;
  }
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kScoreMax = 0x7fffffff;

pcgx_status score_check(const char *fn, const pcgx_kdtree *t, const void *src, int64_t n, const void *poses, int64_t K,
                        float max_dist) {
  if (!t) return fail(PCGX_E_INVALID, "%s: NULL tree", fn);
  if (n < 0 || K < 0) return fail(PCGX_E_INVALID, "%s: negative count", fn);
  if (n > kScoreMax || K > kScoreMax) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points or poses", fn);
  if ((n > 0 && !src) || (K > 0 && !poses)) return fail(PCGX_E_INVALID, "%s: NULL array", fn);
  if (!(max_dist > 0.0f) || !(max_dist < __builtin_inff()))
    return fail(PCGX_E_INVALID, "%s: max_dist must be finite and > 0", fn);
  return PCGX_OK;
}

// PCGX_SCORE_CHUNK=<poses>: the poses a round of launches scores, forced (tests, measurements).  Read per call.
int64_t score_forced_chunk() {
  const char *e = getenv("PCGX_SCORE_CHUNK");
  if (!e || !*e) return 0;
  const long v = atol(e);
  return v > 0 ? (int64_t)v : 0;
}

pcgx_status select_check(const char *fn, const void *status, const void *counts, const void *poses, int64_t n_hyp,
                         int64_t K, const void *ids, const void *out_poses, const void *n_selected) {
  if (n_hyp < 0 || K < 0) return fail(PCGX_E_INVALID, "%s: negative count", fn);
  if (n_hyp > kScoreMax || K > kScoreMax) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 hypotheses or slots", fn);
  if (n_hyp > 0 && (!status || !counts || !poses)) return fail(PCGX_E_INVALID, "%s: NULL input", fn);
  if (K > 0 && (!ids || !out_poses)) return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  if (!n_selected) return fail(PCGX_E_INVALID, "%s: NULL n_selected", fn);
  return PCGX_OK;
}

}  // namespace

extern "C" int32_t pcgx_score_tile(void) { return kScoreTile; }

extern "C" pcgx_status pcgx_kdtree_score_poses_dev(const pcgx_kdtree *t, const float *d_src_xyz, int64_t n,
                                                   const float *d_poses, int64_t K, float max_dist, int32_t *d_counts,
                                                   double *d_sums, void *d_result, void *stream) {
  PCGX_API_LOCK();
  const char *fn = "pcgx_kdtree_score_poses_dev";
  PCGX_TRY(score_check(fn, t, d_src_xyz, n, d_poses, K, max_dist));
  if (!d_result) return fail(PCGX_E_INVALID, "%s: NULL result", fn);
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  const float max_range_sq = max_dist * max_dist;  // as pcgx_kdtree_nearest_batch forms it (kdtree.go:91)
  ScoreInputs in;
  in.n = n;
  in.K = K;
  in.grid = grid_enabled(t);
  in.deletions = t->n_deleted > 0;
  in.empty = t->n_deleted >= t->n;
  in.forced_chunk = score_forced_chunk();
  in.sort_workspace = n > 1 ? radix_sort_workspace_bytes(n) : 0;
  in.have_counts = d_counts != nullptr;
  in.have_sums = d_sums != nullptr;
  const ScorePlan pl = plan_score(in);
  Arena &ar = ctx().arena;
  PCGX_TRY(ar.begin(st));
  void *buf[kScoreBufs] = {};
  for (int b = 0; b < kScoreBufs; b++)
    if (pl.bytes[b]) PCGX_TRY(ar.alloc(pl.bytes[b], &buf[b]));
  if (!d_counts) d_counts = (int32_t *)buf[kBufCounts];
  if (!d_sums) d_sums = (double *)buf[kBufSums];
  const uint32_t ntiles = (uint32_t)pl.tiles;
  ScorePartial *partials = (ScorePartial *)buf[kBufPartials];
  if (pl.path == kScoreNothing || pl.path == kScoreEmpty) {
    if (K > 0) {
      PCGX_HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)K * 4, st));
      PCGX_HIP_TRY(hipMemsetAsync(d_sums, 0, (size_t)K * 8, st));
    }
  } else if (pl.path == kScorePlain) {
    float *q = (float *)buf[kBufPlainQ];
    int32_t *ids = (int32_t *)buf[kBufPlainIds];
    float *dsq = (float *)buf[kBufPlainDsq];
    TreeView tv;
    if (!in.deletions) tv = t->view();
    for (int64_t k = 0; k < K; k++) {
      hipLaunchKernelGGL(score_transform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_src_xyz, n,
                         d_poses + 16 * k, q);
      if (in.deletions)  // the reference's patched tree, as pcgx_kdtree_nearest_batch_dev walks it
        PCGX_TRY(xtree_launch_nearest(t, q, nullptr, n, max_range_sq, 0.0f, ids, dsq, st));
      else
        PCGX_TRY(launch_nearest(tv, q, nullptr, n, max_range_sq, 0.0f, ids, dsq, st));
      hipLaunchKernelGGL(score_count_kernel, dim3(ntiles), dim3(kScoreTile), 0, st, (const float *)q, n,
                         (const int32_t *)ids, (const float *)dsq, partials);
      hipLaunchKernelGGL(score_reduce_kernel, dim3(1), dim3(kScoreTile), 0, st, (const ScorePartial *)partials, ntiles,
                         d_counts + k, d_sums + k);
    }
  } else {
    float4 *src4 = (float4 *)buf[kBufSrc4];
    const uint32_t *order = nullptr;
    if (pl.order) {
      float *box6 = (float *)buf[kBufBox];
      PCGX_TRY(launch_minmax(d_src_xyz, n, 12, 0, box6, st, false));
      uint32_t *keys[2] = {(uint32_t *)buf[kBufKeys0], (uint32_t *)buf[kBufKeys1]};
      uint32_t *vals[2] = {(uint32_t *)buf[kBufVals0], (uint32_t *)buf[kBufVals1]};
      hipLaunchKernelGGL(score_key_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_src_xyz, n,
                         (const float *)box6, keys[0]);
      int res = 0;
      PCGX_TRY(radix_sort_pairs(keys, vals, n, 3 * kScoreKeyBits, buf[kBufSortWs], &res, st, true));
      order = vals[res];
    }
    hipLaunchKernelGGL(score_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_src_xyz, n, order,
                       src4);
    unsigned long long *masks = (unsigned long long *)buf[kBufMasks];
    float *wq = (float *)buf[kBufWalkQ];
    int32_t *wlist = (int32_t *)buf[kBufWalkList], *wids = (int32_t *)buf[kBufWalkIds];
    float *wdsq = (float *)buf[kBufWalkDsq];
    uint32_t *wcount = (uint32_t *)buf[kBufWalkCount];
    PCGX_HIP_TRY(hipMemsetAsync(wcount, 0, pl.bytes[kBufWalkCount], st));
    const TreeView tv = t->view();
    for (int64_t r = 0; r < pl.nchunks; r++) {
      const int64_t k0 = r * pl.chunk, kn = std::min(pl.chunk, K - k0);
      hipLaunchKernelGGL(score_fused_kernel, dim3(xcd_grid(ntiles), (unsigned)kn), dim3(kScoreTile), 0, st, t->grid,
                         (const float4 *)src4, (int32_t)n, ntiles, d_poses + 16 * k0, max_range_sq, partials, masks, wq,
                         wlist, wcount + r);
      PCGX_HIP_TRY(hipGetLastError());
      PCGX_TRY(launch_nearest_listed(tv, wq, wlist, wcount + r, kn * n, max_range_sq, wids, wdsq, st));
      hipLaunchKernelGGL(score_walk_add_kernel, dim3(ntiles, (unsigned)kn), dim3(kScoreTile), 0, st, (int32_t)n, ntiles,
                         (const unsigned long long *)masks, (const int32_t *)wids, (const float *)wdsq, partials);
      hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)kn), dim3(kScoreTile), 0, st,
                         (const ScorePartial *)partials, ntiles, d_counts + k0, d_sums + k0);
    }
  }
  hipLaunchKernelGGL(score_finish_kernel, dim3(1), dim3(kScoreTile), 0, st, d_poses, (int32_t)K, (int32_t)n,
                     (const int32_t *)d_counts, (const double *)d_sums, (int32_t *)d_result);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_kdtree_score_poses(const pcgx_kdtree *t, const float *src_xyz, int64_t n, const float *poses,
                                               int64_t K, float max_dist, int64_t *counts, double *sum_dist_sq,
                                               int64_t *best, float pose16[16]) {
  PCGX_API_CALL();
  const char *fn = "pcgx_kdtree_score_poses";
  PCGX_TRY(score_check(fn, t, src_xyz, n, poses, K, max_dist));
  if (K > 0 && !counts) return fail(PCGX_E_INVALID, "%s: NULL counts", fn);
  if (!best || !pose16) return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_src = nullptr, *d_poses = nullptr;
  int32_t *d_counts = nullptr, *d_result = nullptr;
  double *d_sums = nullptr;
  PCGX_TRY(ha.alloc_n((size_t)(n > 0 ? n : 1) * 3, &d_src));
  PCGX_TRY(ha.alloc_n((size_t)(K > 0 ? K : 1) * 16, &d_poses));
  PCGX_TRY(ha.alloc_n((size_t)(K > 0 ? K : 1), &d_sums));
  PCGX_TRY(ha.alloc_n((size_t)(K > 0 ? K : 1), &d_counts));
  PCGX_TRY(ha.alloc_n((size_t)PCGX_SCORE_RESULT_WORDS, &d_result));
  if (n > 0) PCGX_TRY(staged_upload(d_src, src_xyz, (size_t)n * 12, st));
  if (K > 0) PCGX_TRY(staged_upload(d_poses, poses, (size_t)K * 64, st));
  PCGX_TRY(pcgx_kdtree_score_poses_dev(t, n > 0 ? d_src : nullptr, n, K > 0 ? d_poses : nullptr, K, max_dist, d_counts,
                                       d_sums, d_result, st));
  int32_t r[PCGX_SCORE_RESULT_WORDS];
  PCGX_TRY(staged_download(r, d_result, sizeof r, st));
  *best = r[0];
  memcpy(pose16, &r[8], 64);
  if (K > 0) {
    RawVector<int32_t> c((size_t)K);
    PCGX_TRY(staged_download(c.data(), d_counts, (size_t)K * 4, st));
    for (int64_t k = 0; k < K; k++) counts[k] = c[(size_t)k];
    if (sum_dist_sq) PCGX_TRY(staged_download(sum_dist_sq, d_sums, (size_t)K * 8, st));
  }
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_pose_select_dev(const int32_t *d_status, const int32_t *d_counts, const float *d_poses,
                                            int64_t n_hyp, int64_t K, int32_t *d_ids, float *d_out_poses,
                                            int32_t *d_n_selected, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(select_check("pcgx_pose_select_dev", d_status, d_counts, d_poses, n_hyp, K, d_ids, d_out_poses, d_n_selected));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  hipLaunchKernelGGL(pose_select_kernel, dim3(1), dim3(kSelectBlock), 0, st, d_status, d_counts, d_poses, (int32_t)n_hyp,
                     (int32_t)K, d_ids, d_out_poses, d_n_selected);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_pose_select(const int32_t *status, const int64_t *counts, const float *poses, int64_t n_hyp,
                                        int64_t K, int64_t *ids, float *out_poses, int64_t *n_selected) {
  PCGX_TRY(select_check("pcgx_pose_select", status, counts, poses, n_hyp, K, ids, out_poses, n_selected));
  std::vector<int64_t> okh;
  for (int64_t h = 0; h < n_hyp; h++)
    if (status[h] == 0 && counts[h] >= 3) okh.push_back(h);
  const size_t take = std::min<size_t>(okh.size(), (size_t)K);
  // the first `take` by count descending, then h ascending
  std::partial_sort(okh.begin(), okh.begin() + (ptrdiff_t)take, okh.end(), [&](int64_t a, int64_t b) {
    return counts[a] != counts[b] ? counts[a] > counts[b] : a < b;
  });
  for (int64_t j = 0; j < K; j++) {
    const bool on = (size_t)j < take;
    ids[j] = on ? okh[(size_t)j] : -1;
    for (int i = 0; i < 16; i++) out_poses[16 * j + i] = on ? poses[16 * okh[(size_t)j] + i] : 0.0f;
  }
  *n_selected = (int64_t)take;
  return PCGX_OK;
}
