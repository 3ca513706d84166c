// pose.hip -- the rigid pose most correspondences agree on, by sample consensus over the caller's samples (extension: no
// reference parity; include/pcgx.h, "pose from correspondences").  The shape of sac.hip: the caller draws every random
// number, one call fits and scores all hypotheses and returns the first best.
//   pose_gather_kernel  one thread per pair: its two points into one 32-byte record {p, 0, q, 0}, so that the hot loop
//                       reads memory in order.  A pair with an id out of range, or behind the list's end, is all NaN:
//                       never an inlier.
//   pose_fit_kernel     one lane per hypothesis: pose_terms.h's pose_hypothesis -> status and pose.  Not hot.
//   pose_count_kernel   the hot one: hypotheses x pairs.  One wave per workgroup, TWO hypotheses per lane, their 12 + 12
//                       pose numbers in registers as 12 pairs, so that every multiplication, addition and subtraction
//                       is one packed float32 instruction over both -- each half rounded on its own, the same bits as
//                       two plain ones.  The pair record is wave-uniform: the compiler takes it through scalar loads,
//                       8 SGPRs, no LDS, no cross-lane traffic.  blockIdx.y is the chunk of the pairs (hypothesis waves
//                       alone do not fill the chip); a chunk's counts are added to counts[] by integer atomics, which
//                       give the same sum in any order.  A wave whose hypotheses are all rejected leaves at once.
//                       mat4_transform's w is left out: a status-0 pose has the bottom row 0 0 0 1, so w is exactly 1
//                       for a finite point and x * 1 == x; for a point that is not finite both forms give a DistSq that
//                       is inf or NaN -- never an inlier either way.
//   pose_finish_kernel  ONE workgroup: the first best hypothesis (a max over (count + 1) << 32 | ~h, no atomics), its
//                       inliers compacted in ascending k (wave scans by DPP, the waves' totals through LDS, as
//                       fpfh_corr_kernel), the float64 moments of the inliers about the first one (per thread in
//                       ascending k, then a fixed tree over the lanes, then the waves in ascending order: the same
//                       bits on every call), one lane's solve, the recount under the refined pose and, where that
//                       pose is kept, its inlier list.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "pcgx_internal.h"
#include "pose_terms.h"

namespace pcgx {

constexpr int kPoseBlock = 64;               // one wave per workgroup
constexpr int kPoseTile = 2 * kPoseBlock;    // hypotheses per workgroup: lane l has tile * 128 + l and + 64 + l
constexpr int kPoseTargetWaves = 65536;      // the split makes about this many waves
constexpr int kPoseMinChunk = 256;           // ... but leaves a chunk at least this many pairs
constexpr int kPoseMaxSplit = 65535;         // gridDim.y
constexpr int kFinishBlock = 1024;
constexpr int kFinishWaves = kFinishBlock / 64;
constexpr int kResultWords = PCGX_POSE_RESULT_WORDS;

typedef float pose_f2 __attribute__((ext_vector_type(2)));

// the length of the list: m_cap, or what the device word says, held to [0, m_cap]
__device__ __forceinline__ int32_t pose_list_len(const int32_t *__restrict__ d_n_pairs, int32_t m_cap) {
  if (!d_n_pairs) return m_cap;
  const int32_t m = *d_n_pairs;
  return m < 0 ? 0 : (m > m_cap ? m_cap : m);
}

__global__ __launch_bounds__(256) void pose_gather_kernel(const float *__restrict__ src_xyz, int64_t ns,
                                                          const float *__restrict__ dst_xyz, int64_t nd,
                                                          const int32_t *__restrict__ src_ids,
                                                          const int32_t *__restrict__ dst_ids, int32_t m_cap,
                                                          const int32_t *__restrict__ d_n_pairs,
                                                          float4 *__restrict__ recs) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m_cap) return;
  const float nan = __builtin_nanf("");
  float4 p = {nan, nan, nan, 0.0f}, q = {nan, nan, nan, 0.0f};
  if (k < pose_list_len(d_n_pairs, m_cap)) {
    const int64_t s = src_ids[k], d = dst_ids[k];
    if (s >= 0 && s < ns && d >= 0 && d < nd) {
      p = float4{src_xyz[3 * s], src_xyz[3 * s + 1], src_xyz[3 * s + 2], 0.0f};
      q = float4{dst_xyz[3 * d], dst_xyz[3 * d + 1], dst_xyz[3 * d + 2], 0.0f};
    }
  }
  recs[2 * k] = p;
  recs[2 * k + 1] = q;
}

__global__ __launch_bounds__(256) void pose_fit_kernel(const float *__restrict__ src_xyz, int64_t ns,
                                                       const float *__restrict__ dst_xyz, int64_t nd,
                                                       const int32_t *__restrict__ src_ids,
                                                       const int32_t *__restrict__ dst_ids, int32_t m_cap,
                                                       const int32_t *__restrict__ d_n_pairs,
                                                       const uint32_t *__restrict__ samples, int64_t n_hyp,
                                                       float edge_similarity, int32_t *__restrict__ status,
                                                       float *__restrict__ poses) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n_hyp) return;
  const uint32_t u[3] = {samples[3 * h], samples[3 * h + 1], samples[3 * h + 2]};
  float pose[16];
  status[h] = pose_hypothesis(src_xyz, ns, dst_xyz, nd, src_ids, dst_ids, pose_list_len(d_n_pairs, m_cap), u,
                              edge_similarity, pose);
#pragma unroll
  for (int i = 0; i < 16; i++) poses[16 * h + i] = pose[i];  // (the caller's array: no alignment beyond a float's)
}

__global__ __launch_bounds__(kPoseBlock) void pose_count_kernel(const float4 *__restrict__ recs, int32_t m_cap,
                                                                const int32_t *__restrict__ d_n_pairs, int64_t n_hyp,
                                                                const int32_t *__restrict__ status,
                                                                const float *__restrict__ poses, float max_dist_sq,
                                                                int32_t chunk, int32_t *__restrict__ counts) {
  const int64_t h0 = (int64_t)blockIdx.x * kPoseTile + threadIdx.x, h1 = h0 + kPoseBlock;
  const bool ok0 = h0 < n_hyp && status[h0] == kPoseOk, ok1 = h1 < n_hyp && status[h1] == kPoseOk;
  if (__ballot(ok0 || ok1) == 0ull) return;  // (wave-uniform)
  const float *a = poses + 16 * (h0 < n_hyp ? h0 : n_hyp - 1), *b = poses + 16 * (h1 < n_hyp ? h1 : n_hyp - 1);
  pose_f2 m[12];  // column c, row r at 3 c + r
#pragma unroll
  for (int c = 0; c < 4; c++)
#pragma unroll
    for (int r = 0; r < 3; r++) m[3 * c + r] = pose_f2{a[4 * c + r], b[4 * c + r]};
  const int32_t len = pose_list_len(d_n_pairs, m_cap);
  const int64_t k0 = (int64_t)blockIdx.y * chunk;
  const int64_t k1 = k0 + chunk < len ? k0 + chunk : len;
  int32_t c0 = 0, c1 = 0;
#pragma unroll 4  // (four records' scalar loads in flight ahead of their arithmetic)
  for (int64_t k = k0; k < k1; k++) {
    const float4 p = recs[2 * k], q = recs[2 * k + 1];  // (wave-uniform: scalar loads)
    const pose_f2 px = {p.x, p.x}, py = {p.y, p.y}, pz = {p.z, p.z};
    const pose_f2 x = ((m[0] * px + m[3] * py) + m[6] * pz) + m[9];
    const pose_f2 y = ((m[1] * px + m[4] * py) + m[7] * pz) + m[10];
    const pose_f2 z = ((m[2] * px + m[5] * py) + m[8] * pz) + m[11];
    const pose_f2 dx = pose_f2{q.x, q.x} - x, dy = pose_f2{q.y, q.y} - y, dz = pose_f2{q.z, q.z} - z;
    const pose_f2 D = (dx * dx + dy * dy) + dz * dz;
    c0 += D.x < max_dist_sq ? 1 : 0;
    c1 += D.y < max_dist_sq ? 1 : 0;
  }
  if (ok0 && c0) atomicAdd(&counts[h0], c0);
  if (ok1 && c1) atomicAdd(&counts[h1], c1);
}

// ---- the one-workgroup tail

struct FinishShared {
  uint64_t u64[kFinishWaves];
  uint32_t u32[kFinishWaves];
  double mom[kFinishWaves][16];
  float pose[16], refit[16];
  int32_t refit_ok;
};

// the largest key of the workgroup, in every thread (all threads must be here)
__device__ __forceinline__ uint64_t finish_max_u64(uint64_t v, FinishShared &s) {
  const int t = (int)threadIdx.x;
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    const uint64_t o = __shfl_xor(v, x);
    v = o > v ? o : v;
  }
  if ((t & 63) == 0) s.u64[t >> 6] = v;
  __syncthreads();
  uint64_t r = 0;
#pragma unroll
  for (int w = 0; w < kFinishWaves; w++) r = s.u64[w] > r ? s.u64[w] : r;
  __syncthreads();
  return r;
}

// The pairs k < len that are inliers under `pose`, in ascending k: their number, in every thread; with ids != NULL the
// list too, -1 from its end to m_cap.  (all threads must be here)
__device__ __forceinline__ uint32_t finish_inliers(const float *pose, const float4 *__restrict__ recs, int32_t len,
                                                   int32_t m_cap, float max_dist_sq, int32_t *__restrict__ ids,
                                                   FinishShared &s) {
  const int t = (int)threadIdx.x, wave = t >> 6;
  uint32_t base = 0u;  // inliers before this round (the same in every thread)
  for (int64_t k0 = 0; k0 < len; k0 += kFinishBlock) {
    const int64_t k = k0 + t;
    bool in = false;
    if (k < len) {
      const float4 p = recs[2 * k], q = recs[2 * k + 1];
      in = pose_dist_sq(pose, &p.x, &q.x) < max_dist_sq;
    }
    const uint32_t incl = wave_incl_scan_u32(in ? 1u : 0u);
    if ((t & 63) == 63) s.u32[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < kFinishWaves; w++) {
      const uint32_t c = s.u32[w];
      before += w < wave ? c : 0u;
      total += c;
    }
    __syncthreads();
    if (in && ids) ids[base + before + incl - 1u] = (int32_t)k;
    base += total;
  }
  if (ids)
    for (int64_t i = (int64_t)base + t; i < m_cap; i += kFinishBlock) ids[i] = -1;
  return base;
}

__global__ __launch_bounds__(kFinishBlock) void pose_finish_kernel(const float4 *__restrict__ recs, int32_t m_cap,
                                                                   const int32_t *__restrict__ d_n_pairs, int64_t n_hyp,
                                                                   const int32_t *__restrict__ status,
                                                                   const int32_t *__restrict__ counts,
                                                                   const float *__restrict__ poses, float max_dist_sq,
                                                                   int32_t refine, int32_t *__restrict__ ids,
                                                                   int32_t *__restrict__ result) {
  __shared__ FinishShared s;
  const int t = (int)threadIdx.x, wave = t >> 6;
  const int32_t len = pose_list_len(d_n_pairs, m_cap);
  // the first best: the largest count, the smallest h among equals; 0: no hypothesis has status 0
  uint64_t key = 0;
  for (int64_t h = t; h < n_hyp; h += kFinishBlock)
    if (status[h] == kPoseOk) {
      const uint64_t k = ((uint64_t)((uint32_t)counts[h] + 1u) << 32) | (uint64_t)(~(uint32_t)h);
      key = k > key ? k : key;
    }
  key = finish_max_u64(key, s);
  const int32_t best = key ? (int32_t)(~(uint32_t)key) : -1;
  const int32_t best_count = key ? (int32_t)((uint32_t)(key >> 32) - 1u) : 0;
  const bool found = best_count >= 3;
  if (t < 16) s.pose[t] = best >= 0 ? poses[16 * (int64_t)best + t] : 0.0f;
  if (t == 0) s.refit_ok = 0;
  __syncthreads();
  uint32_t n_in = 0u;
  if (best >= 0) {
    n_in = finish_inliers(s.pose, recs, len, m_cap, max_dist_sq, ids, s);
  } else {
    for (int64_t i = t; i < m_cap; i += kFinishBlock) ids[i] = -1;
  }
  int32_t refined = 0;
  if (refine && found && n_in > 0u) {  // (workgroup-uniform)
    __syncthreads();  // the list is in memory
    const int32_t first = ids[0];
    const float4 op = recs[2 * (int64_t)first], oq = recs[2 * (int64_t)first + 1];
    PoseMoments a;
    pose_moments_clear(a);
    for (uint32_t i = (uint32_t)t; i < n_in; i += kFinishBlock) {
      const int64_t k = ids[i];
      const float4 p = recs[2 * k], q = recs[2 * k + 1];
      pose_moments_add(a, &p.x, &q.x, &op.x, &oq.x);
    }
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) {
      a.n += __shfl_xor(a.n, x);
#pragma unroll
      for (int i = 0; i < 3; i++) {
        a.sp[i] += __shfl_xor(a.sp[i], x);
        a.sq[i] += __shfl_xor(a.sq[i], x);
#pragma unroll
        for (int j = 0; j < 3; j++) a.spq[i][j] += __shfl_xor(a.spq[i][j], x);
      }
    }
    if ((t & 63) == 0) {
      double *o = s.mom[wave];
      o[0] = a.n;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        o[1 + i] = a.sp[i];
        o[4 + i] = a.sq[i];
#pragma unroll
        for (int j = 0; j < 3; j++) o[7 + 3 * i + j] = a.spq[i][j];
      }
    }
    __syncthreads();
    if (t == 0) {
      PoseMoments all;
      pose_moments_clear(all);
      for (int w = 0; w < kFinishWaves; w++) {  // ascending
        const double *o = s.mom[w];
        all.n += o[0];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          all.sp[i] += o[1 + i];
          all.sq[i] += o[4 + i];
#pragma unroll
          for (int j = 0; j < 3; j++) all.spq[i][j] += o[7 + 3 * i + j];
        }
      }
      float pose[16];
      double l1, l2;
      const bool solved = pose_solve(all, &op.x, &oq.x, pose, l1, l2);
      for (int i = 0; i < 16; i++) s.refit[i] = pose[i];
      s.refit_ok = pose_refit_allowed(all.n, solved, l1, l2) ? 1 : 0;
    }
    __syncthreads();
    if (s.refit_ok) {
      const uint32_t n2 = finish_inliers(s.refit, recs, len, m_cap, max_dist_sq, nullptr, s);
      if ((int32_t)n2 >= best_count) {  // the refined pose replaces the best's
        refined = 1;
        __syncthreads();  // (every thread has read the old list)
        n_in = finish_inliers(s.refit, recs, len, m_cap, max_dist_sq, ids, s);
      }
    }
  }
  if (t == 0) {
    result[0] = found ? 1 : 0;
    result[1] = best;
    result[2] = best_count;
    result[3] = refined;
    result[4] = (int32_t)n_in;
    result[5] = len;
    result[6] = result[7] = 0;
  }
  if (t < 16) ((float *)result)[8 + t] = refined ? s.refit[t] : s.pose[t];
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kPoseMax = 0x7fffffff;  // ids and counts are int32 on the device

pcgx_status pose_check(const char *fn, const void *src_xyz, int64_t ns, const void *dst_xyz, int64_t nd,
                       const void *src_ids, const void *dst_ids, int64_t m, const void *samples, int64_t n_hyp,
                       float max_dist_sq, float edge_similarity) {
  if (ns < 0 || nd < 0 || m < 0 || n_hyp < 0) return fail(PCGX_E_INVALID, "%s: negative count", fn);
  if (ns > kPoseMax || nd > kPoseMax || m > kPoseMax || n_hyp > kPoseMax)
    return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points, pairs or hypotheses", fn);
  if ((ns > 0 && !src_xyz) || (nd > 0 && !dst_xyz)) return fail(PCGX_E_INVALID, "%s: NULL points", fn);
  if (m > 0 && (!src_ids || !dst_ids)) return fail(PCGX_E_INVALID, "%s: NULL ids", fn);
  if (n_hyp > 0 && !samples) return fail(PCGX_E_INVALID, "%s: NULL samples", fn);
  if (!(max_dist_sq > 0.0f) || !(max_dist_sq < __builtin_inff()))
    return fail(PCGX_E_INVALID, "%s: max_dist_sq must be finite and > 0", fn);
  if (!(edge_similarity >= 0.0f) || !(edge_similarity <= 1.0f))
    return fail(PCGX_E_INVALID, "%s: edge_similarity must be in [0, 1]", fn);
  return PCGX_OK;
}

// PCGX_POSE_SPLIT=<n>: the number of chunks of the pairs, forced (tests of the merge, measurements).  Read per call.
int32_t pose_split(int64_t n_hyp, int64_t m_cap) {
  const char *e = getenv("PCGX_POSE_SPLIT");
  if (e && *e) {
    const long v = atol(e);
    if (v > 0) return (int32_t)(v < kPoseMaxSplit ? v : kPoseMaxSplit);
  }
  const int64_t tiles = (n_hyp + kPoseTile - 1) / kPoseTile;
  int64_t s = (kPoseTargetWaves + tiles - 1) / tiles;
  const int64_t cap = m_cap / kPoseMinChunk;
  if (s > cap) s = cap;
  if (s > kPoseMaxSplit) s = kPoseMaxSplit;
  return (int32_t)(s < 1 ? 1 : s);
}

}  // namespace

extern "C" int32_t pcgx_pose_tile(void) { return kPoseTile; }

extern "C" pcgx_status pcgx_pose_from_correspondences_dev(const float *d_src_xyz, int64_t ns, const float *d_dst_xyz,
                                                          int64_t nd, const int32_t *d_src_ids,
                                                          const int32_t *d_dst_ids, int64_t m_cap,
                                                          const int32_t *d_n_pairs, const uint32_t *d_samples,
                                                          int64_t n_hyp, float max_dist_sq, float edge_similarity,
                                                          int32_t refine, void *d_result, int32_t *d_inlier_ids,
                                                          int32_t *d_status, int32_t *d_counts, float *d_poses,
                                                          void *stream) {
  PCGX_API_LOCK();
  const char *fn = "pcgx_pose_from_correspondences_dev";
  PCGX_TRY(pose_check(fn, d_src_xyz, ns, d_dst_xyz, nd, d_src_ids, d_dst_ids, m_cap, d_samples, n_hyp, max_dist_sq,
                      edge_similarity));
  if (!d_result) return fail(PCGX_E_INVALID, "%s: NULL result", fn);
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  Arena &ar = ctx().arena;
  PCGX_TRY(ar.begin(st));
  const int32_t mc = (int32_t)m_cap;
  float4 *recs = nullptr;
  PCGX_TRY(ar.alloc_n((size_t)(m_cap > 0 ? m_cap : 1) * 2, &recs));
  if (!d_inlier_ids) PCGX_TRY(ar.alloc_n((size_t)(m_cap > 0 ? m_cap : 1), &d_inlier_ids));
  if (!d_status) PCGX_TRY(ar.alloc_n((size_t)(n_hyp > 0 ? n_hyp : 1), &d_status));
  if (!d_counts) PCGX_TRY(ar.alloc_n((size_t)(n_hyp > 0 ? n_hyp : 1), &d_counts));
  if (!d_poses) PCGX_TRY(ar.alloc_n((size_t)(n_hyp > 0 ? n_hyp : 1) * 16, &d_poses));
  if (m_cap > 0)
    hipLaunchKernelGGL(pose_gather_kernel, dim3((unsigned)((m_cap + 255) / 256)), dim3(256), 0, st, d_src_xyz, ns,
                       d_dst_xyz, nd, d_src_ids, d_dst_ids, mc, d_n_pairs, recs);
  if (n_hyp > 0) {
    PCGX_HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)n_hyp * sizeof(int32_t), st));
    hipLaunchKernelGGL(pose_fit_kernel, dim3((unsigned)((n_hyp + 255) / 256)), dim3(256), 0, st, d_src_xyz, ns, d_dst_xyz,
                       nd, d_src_ids, d_dst_ids, mc, d_n_pairs, d_samples, n_hyp, edge_similarity, d_status, d_poses);
    if (m_cap > 0) {
      const int32_t split = pose_split(n_hyp, m_cap);
      int64_t chunk = (m_cap + split - 1) / split;
      if (chunk < 1) chunk = 1;
      const dim3 grid((unsigned)((n_hyp + kPoseTile - 1) / kPoseTile), (unsigned)split);
      hipLaunchKernelGGL(pose_count_kernel, grid, dim3(kPoseBlock), 0, st, (const float4 *)recs, mc, d_n_pairs, n_hyp,
                         (const int32_t *)d_status, (const float *)d_poses, max_dist_sq, (int32_t)chunk, d_counts);
    }
  }
  hipLaunchKernelGGL(pose_finish_kernel, dim3(1), dim3(kFinishBlock), 0, st, (const float4 *)recs, mc, d_n_pairs, n_hyp,
                     (const int32_t *)d_status, (const int32_t *)d_counts, (const float *)d_poses, max_dist_sq, refine,
                     d_inlier_ids, (int32_t *)d_result);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_pose_from_correspondences(const float *src_xyz, int64_t ns, const float *dst_xyz, int64_t nd,
                                                      const int64_t *src_ids, const int64_t *dst_ids, int64_t m,
                                                      const uint32_t *samples, int64_t n_hyp, float max_dist_sq,
                                                      float edge_similarity, int32_t refine, int32_t *found,
                                                      int64_t *best, int64_t *best_count, float *pose16,
                                                      int32_t *refined, int64_t *n_inliers, int64_t *inlier_ids,
                                                      int32_t *status, int64_t *counts, float *poses) {
  PCGX_API_CALL();
  const char *fn = "pcgx_pose_from_correspondences";
  PCGX_TRY(pose_check(fn, src_xyz, ns, dst_xyz, nd, src_ids, dst_ids, m, samples, n_hyp, max_dist_sq, edge_similarity));
  if (!found || !best || !best_count || !pose16 || !refined || !n_inliers) return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  for (int64_t k = 0; k < m; k++)
    if (src_ids[k] < 0 || src_ids[k] >= ns || dst_ids[k] < 0 || dst_ids[k] >= nd)
      return fail(PCGX_E_INVALID, "%s: pair %lld names a point out of range", fn, (long long)k);
  *found = 0;
  *best = -1;
  *best_count = 0;
  *refined = 0;
  *n_inliers = 0;
  for (int i = 0; i < 16; i++) pose16[i] = 0.0f;
  if (n_hyp == 0 || m == 0) {
    if (inlier_ids)
      for (int64_t k = 0; k < m; k++) inlier_ids[k] = -1;
    for (int64_t h = 0; h < n_hyp; h++) {
      if (status) status[h] = kPoseBadSample;
      if (counts) counts[h] = 0;
      if (poses)
        for (int i = 0; i < 16; i++) poses[16 * h + i] = 0.0f;
    }
    return PCGX_OK;
  }
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_src = nullptr, *d_dst = nullptr, *d_poses = nullptr;
  int32_t *d_ids = nullptr, *d_out = nullptr, *d_status = nullptr, *d_counts = nullptr;
  uint32_t *d_samples = nullptr;
  PCGX_TRY(ha.alloc_n((size_t)ns * 3, &d_src));
  PCGX_TRY(ha.alloc_n((size_t)nd * 3, &d_dst));
  PCGX_TRY(ha.alloc_n((size_t)m * 2, &d_ids));
  PCGX_TRY(ha.alloc_n((size_t)n_hyp * 3, &d_samples));
  PCGX_TRY(ha.alloc_n((size_t)m + kResultWords, &d_out));  // the record, then the inlier list
  if (status) PCGX_TRY(ha.alloc_n((size_t)n_hyp, &d_status));
  if (counts) PCGX_TRY(ha.alloc_n((size_t)n_hyp, &d_counts));
  if (poses) PCGX_TRY(ha.alloc_n((size_t)n_hyp * 16, &d_poses));
  RawVector<int32_t> h((size_t)m * 2);
  for (int64_t k = 0; k < m; k++) {
    h[(size_t)k] = (int32_t)src_ids[k];
    h[(size_t)(m + k)] = (int32_t)dst_ids[k];
  }
  PCGX_TRY(staged_upload(d_src, src_xyz, (size_t)ns * 12, st));
  PCGX_TRY(staged_upload(d_dst, dst_xyz, (size_t)nd * 12, st));
  PCGX_TRY(staged_upload(d_ids, h.data(), (size_t)m * 8, st));
  PCGX_TRY(staged_upload(d_samples, samples, (size_t)n_hyp * 12, st));
  PCGX_TRY(pcgx_pose_from_correspondences_dev(d_src, ns, d_dst, nd, d_ids, d_ids + m, m, nullptr, d_samples, n_hyp,
                                              max_dist_sq, edge_similarity, refine, d_out, d_out + kResultWords,
                                              d_status, d_counts, d_poses, st));
  RawVector<int32_t> r((size_t)m + kResultWords);
  PCGX_TRY(staged_download(r.data(), d_out, ((size_t)m + kResultWords) * 4, st));
  *found = r[0];
  *best = r[1];
  *best_count = r[2];
  *refined = r[3];
  *n_inliers = r[4];
  memcpy(pose16, &r[8], 64);
  if (inlier_ids)
    for (int64_t k = 0; k < m; k++) inlier_ids[k] = r[(size_t)(kResultWords + k)];
  if (status) PCGX_TRY(staged_download(status, d_status, (size_t)n_hyp * 4, st));
  if (poses) PCGX_TRY(staged_download(poses, d_poses, (size_t)n_hyp * 64, st));
  if (counts) {
    RawVector<int32_t> c((size_t)n_hyp);
    PCGX_TRY(staged_download(c.data(), d_counts, (size_t)n_hyp * 4, st));
    for (int64_t i = 0; i < n_hyp; i++) counts[i] = c[(size_t)i];
  }
  return PCGX_OK;
}
