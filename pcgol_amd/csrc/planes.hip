// planes.hip -- plane segmentation: the plane most of the cloud agrees on, by sample consensus over the caller's samples,
// its inliers taken out, then the next one (extension: no reference parity; include/pcgx.h, "planes").  The contract of
// pose.hip: the caller draws every random word, one call fits and scores all hypotheses, the first best wins.  All
// max_planes rounds are enqueued up front; a round reads from device words (PlaneState) how many points are left and
// whether an earlier round failed, and every kernel of a round that does not run returns at once.  No kernel waits on
// another workgroup.
//
// A round works on the points that are left, A_r, as a list of ids in ascending order with their records compacted
// beside it (16 bytes a point, 16 more with normals): the count kernel reads R_r records, not Len().
//   planes_gather_kernel      once: a lane per id, the point (and its normal) into records, NaN where the point is not
//                             live; labels and ids to -1.
//   planes_fit_kernel         a lane per hypothesis: plane_terms.h's plane_hypothesis -> status and plane, count 0.
//   planes_count_kernel       the hot one, hypotheses x points: pose_count_kernel's shape.  One wave per workgroup, TWO
//                             hypotheses per lane, their four numbers as packed float32 pairs (each half rounded on its
//                             own: the bits of two plain operations), the point record wave-uniform through scalar
//                             loads, blockIdx.y over chunks of the list, an integer atomicAdd per lane at the end.  No LDS.
//   planes_select_kernel      ONE workgroup: the first best (a max over (count + 1) << 32 | ~h), found or not.
//   planes_tile_count_kernel  the ordered compaction, three kernels (many workgroups, one for the tile offsets): how many
//   planes_scan_kernel        entries of each tile of 1024 leave (init: are not live; else: are inliers of the round's
//   planes_scatter_kernel     plane), the exclusive scan of that, and the scatter: those that leave to the inlier list in
//                             order, those that stay to the next round's list and records in order.
//   planes_refit_kernel       one lane: plane_terms.h's plane_refit from group geometry's answer (group_stats.hip's own
//                             kernels, enqueued on the candidate inlier list with its size in a device word).
//   planes_round_end_kernel   one lane: the round's row of the outputs, and the state of the next round.
// Integer atomics only: the same input gives the same bits on every call, whatever the split.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "group_list.h"
#include "plane_terms.h"

namespace pcgx {

constexpr int kPlBlock = 64;              // one wave per workgroup
constexpr int kPlTile = 2 * kPlBlock;     // hypotheses per workgroup: lane l has tile * 128 + l and + 64 + l
constexpr int kPlTargetWaves = 65536;     // the split makes about this many waves (as pose.hip)
constexpr int kPlMinChunk = 256;          // ... but leaves a chunk at least this many points
constexpr int kPlMaxSplit = 65535;        // gridDim.y
constexpr int kCpBlock = 256, kCpIters = 4;
constexpr int kCpTile = kCpBlock * kCpIters;  // entries per workgroup of the compaction
constexpr int kOneBlock = 1024;               // the one-workgroup kernels
constexpr int kOneWaves = kOneBlock / 64;

typedef float plane_f2 __attribute__((ext_vector_type(2)));

// The device words the rounds hand on.
struct PlaneState {
  int32_t run;         // this round runs
  int32_t R;           // |A_r|
  int32_t off;         // inliers of the earlier rounds: where this round's go in ids
  int32_t found;       // the round found a plane (select)
  int32_t best, best_count;
  int32_t cand_size;   // the size word group geometry reads: the best hypothesis's inliers, 0 when nothing is refitted
  int32_t refit_ok;    // plane[1] is a refitted plane
  int32_t use;         // the kept plane: 0 the hypothesis's, 1 the refitted one
  int32_t total[2];    // the inliers of plane[0] and plane[1]
  int32_t pad;
  float plane[2][4];
};

enum { kInit = 0, kHyp = 1, kRefit = 2 };     // what a tile count / scan is for
enum { kToFirst = 0, kToCand = 1, kToNext = 2 };  // ... and a scatter

__global__ __launch_bounds__(256) void planes_gather_kernel(const float4 *__restrict__ nodes, const uint32_t *__restrict__ inv,
                                                            int32_t n, const uint8_t *__restrict__ deleted,
                                                            const float *__restrict__ normals, float4 *__restrict__ P,
                                                            float4 *__restrict__ N, int32_t *__restrict__ labels,
                                                            int32_t *__restrict__ ids) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float nan = __builtin_nanf("");
  const float4 nd = node_at(nodes, inv[i]);
  bool live = !(deleted && deleted[i]) && plane_point_live(nd.x, nd.y, nd.z);
  float4 m = {0.0f, 0.0f, 0.0f, 0.0f};
  if (normals) {
    m = float4{normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], 0.0f};
    live = live && plane_normal_live(m.x, m.y, m.z);
  }
  P[i] = live ? float4{nd.x, nd.y, nd.z, 0.0f} : float4{nan, nan, nan, 0.0f};
  if (N) N[i] = live ? m : float4{nan, nan, nan, 0.0f};
  labels[i] = -1;
  ids[i] = -1;
}

// n_hyp == 0 or Len() == 0: nothing runs, every row of every output is written
__global__ __launch_bounds__(256) void planes_empty_kernel(int32_t n, int64_t rows, int32_t max_planes,
                                                           int32_t *__restrict__ d_n_planes, float *__restrict__ planes,
                                                           int32_t *__restrict__ sizes, int32_t *__restrict__ refined,
                                                           int32_t *__restrict__ best, int32_t *__restrict__ labels,
                                                           int32_t *__restrict__ ids, int32_t *__restrict__ status,
                                                           int32_t *__restrict__ counts, float *__restrict__ hyp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *d_n_planes = 0;
  if (i < n) {
    labels[i] = -1;
    if (ids) ids[i] = -1;
  }
  if (i < max_planes) {
    planes[4 * i] = planes[4 * i + 1] = planes[4 * i + 2] = planes[4 * i + 3] = 0.0f;
    sizes[i] = 0;
    refined[i] = 0;
    best[i] = -1;
  }
  if (i < rows) {
    if (status) status[i] = kPlaneNotRun;
    if (counts) counts[i] = 0;
    if (hyp) hyp[4 * i] = hyp[4 * i + 1] = hyp[4 * i + 2] = hyp[4 * i + 3] = 0.0f;
  }
}

__global__ __launch_bounds__(256) void planes_fit_kernel(const PlaneState *__restrict__ S, const float4 *__restrict__ P,
                                                         const uint32_t *__restrict__ samples, int64_t n_hyp, PlaneAxis ax,
                                                         int32_t *__restrict__ status, int32_t *__restrict__ counts,
                                                         float *__restrict__ hyp) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n_hyp) return;
  float pl[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int32_t st = kPlaneNotRun;
  if (S->run) {
    const uint32_t R = (uint32_t)S->R;
    const uint32_t i0 = pose_sample_index(samples[3 * h], R), i1 = pose_sample_index(samples[3 * h + 1], R),
                   i2 = pose_sample_index(samples[3 * h + 2], R);
    const float4 p0 = P[i0], p1 = P[i1], p2 = P[i2];
    st = plane_hypothesis(i0, i1, i2, &p0.x, &p1.x, &p2.x, ax, pl);
  }
  status[h] = st;
  counts[h] = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) hyp[4 * h + k] = pl[k];  // (the caller's array: no alignment beyond a float's)
}

template <bool kNormals>
__global__ __launch_bounds__(kPlBlock) void planes_count_kernel(const PlaneState *__restrict__ S, const float4 *__restrict__ P,
                                                                const float4 *__restrict__ N, int64_t n_hyp,
                                                                const int32_t *__restrict__ status,
                                                                const float *__restrict__ hyp, float max_dist,
                                                                float min_normal_cos, int32_t chunk,
                                                                int32_t *__restrict__ counts) {
  if (!S->run) return;  // (uniform)
  const int64_t h0 = (int64_t)blockIdx.x * kPlTile + threadIdx.x, h1 = h0 + kPlBlock;
  const bool ok0 = h0 < n_hyp && status[h0] == kPlaneOk, ok1 = h1 < n_hyp && status[h1] == kPlaneOk;
  if (__ballot(ok0 || ok1) == 0ull) return;  // (wave-uniform)
  const int64_t len = S->R;
  const int64_t k0 = (int64_t)blockIdx.y * chunk;
  if (k0 >= len) return;
  const int64_t k1 = k0 + chunk < len ? k0 + chunk : len;
  const float *a = hyp + 4 * (h0 < n_hyp ? h0 : n_hyp - 1), *b = hyp + 4 * (h1 < n_hyp ? h1 : n_hyp - 1);
  const plane_f2 nx = {a[0], b[0]}, ny = {a[1], b[1]}, nz = {a[2], b[2]}, d = {a[3], b[3]};
  int32_t c0 = 0, c1 = 0;
#pragma unroll 4  // (four records' scalar loads in flight ahead of their arithmetic)
  for (int64_t k = k0; k < k1; k++) {
    const float4 p = P[k];  // (wave-uniform: a scalar load)
    const plane_f2 s = ((nx * plane_f2{p.x, p.x} + ny * plane_f2{p.y, p.y}) + nz * plane_f2{p.z, p.z}) + d;
    bool in0 = fabsf(s.x) < max_dist, in1 = fabsf(s.y) < max_dist;
    if (kNormals) {
      const float4 m = N[k];
      const plane_f2 c = (nx * plane_f2{m.x, m.x} + ny * plane_f2{m.y, m.y}) + nz * plane_f2{m.z, m.z};
      in0 = in0 && fabsf(c.x) >= min_normal_cos;
      in1 = in1 && fabsf(c.y) >= min_normal_cos;
    }
    c0 += in0 ? 1 : 0;
    c1 += in1 ? 1 : 0;
  }
  if (ok0 && c0) atomicAdd(&counts[h0], c0);
  if (ok1 && c1) atomicAdd(&counts[h1], c1);
}

__global__ __launch_bounds__(kOneBlock) void planes_select_kernel(PlaneState *__restrict__ S, int64_t n_hyp,
                                                                  const int32_t *__restrict__ status,
                                                                  const int32_t *__restrict__ counts,
                                                                  const float *__restrict__ hyp, int64_t min_inliers) {
  __shared__ uint64_t s_key[kOneWaves];
  const int t = (int)threadIdx.x;
  const bool run = S->run != 0;
  // the first best: the largest count, the smallest h among equals; 0: no hypothesis has status 0
  uint64_t key = 0;
  if (run)
    for (int64_t h = t; h < n_hyp; h += kOneBlock)
      if (status[h] == kPlaneOk) {
        const uint64_t k = ((uint64_t)((uint32_t)counts[h] + 1u) << 32) | (uint64_t)(~(uint32_t)h);
        key = k > key ? k : key;
      }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    const uint64_t o = __shfl_xor(key, x);
    key = o > key ? o : key;
  }
  if ((t & 63) == 0) s_key[t >> 6] = key;
  __syncthreads();
  if (t != 0) return;
  key = 0;
  for (int w = 0; w < kOneWaves; w++) key = s_key[w] > key ? s_key[w] : key;
  const int32_t best = key ? (int32_t)(~(uint32_t)key) : -1;
  const int32_t best_count = key ? (int32_t)((uint32_t)(key >> 32) - 1u) : 0;
  const int64_t need = min_inliers > 3 ? min_inliers : 3;
  const bool found = run && key && (int64_t)best_count >= need;
  S->found = found ? 1 : 0;
  S->best = best;
  S->best_count = best_count;
  S->cand_size = 0;
  S->refit_ok = 0;
  S->use = 0;
  S->total[0] = S->total[1] = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    S->plane[0][k] = found ? hyp[4 * (int64_t)best + k] : 0.0f;
    S->plane[1][k] = 0.0f;
  }
}

// ---- the ordered compaction

// does entry i leave the list?  init: it is not live (its record is NaN); else: it is an inlier of pl
template <bool kIsInit>
__device__ __forceinline__ bool planes_leaves(const float4 *__restrict__ P, const float4 *__restrict__ N, int64_t i,
                                              const float *pl, float max_dist, float min_normal_cos) {
  const float4 p = P[i];
  if (kIsInit) return !(p.x == p.x);
  bool in = plane_near(pl, p.x, p.y, p.z, max_dist);
  if (N) {
    const float4 m = N[i];
    in = in && plane_normal_agrees(pl, m.x, m.y, m.z, min_normal_cos);
  }
  return in;
}

template <int kMode>
__global__ __launch_bounds__(kCpBlock) void planes_tile_count_kernel(const PlaneState *__restrict__ S, int32_t n,
                                                                     const float4 *__restrict__ P,
                                                                     const float4 *__restrict__ N, float max_dist,
                                                                     float min_normal_cos, int32_t *__restrict__ tile_cnt) {
  __shared__ int32_t s_w[kCpBlock / 64];
  int64_t len = n;
  float pl[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (kMode != kInit) {
    if (!S->found || (kMode == kRefit && !S->refit_ok)) return;  // (uniform)
    len = S->R;
#pragma unroll
    for (int k = 0; k < 4; k++) pl[k] = S->plane[kMode == kRefit ? 1 : 0][k];
  }
  const int64_t base = (int64_t)blockIdx.x * kCpTile;
  if (base >= len) return;  // (uniform; the scan reads the tiles below len only)
  int32_t c = 0;
#pragma unroll
  for (int j = 0; j < kCpIters; j++) {
    const int64_t i = base + j * kCpBlock + threadIdx.x;
    if (i < len) c += planes_leaves<kMode == kInit>(P, N, i, pl, max_dist, min_normal_cos) ? 1 : 0;
  }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) c += __shfl_xor(c, x);
  if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kCpBlock / 64; w++) sum += s_w[w];
    tile_cnt[blockIdx.x] = sum;
  }
}

// ONE workgroup: tile_off = the exclusive scan of tile_cnt over the tiles of the list, and what the total decides
template <int kMode>
__global__ __launch_bounds__(kOneBlock) void planes_scan_kernel(PlaneState *__restrict__ S, int32_t n, int32_t refine,
                                                                const int32_t *__restrict__ tile_cnt,
                                                                int32_t *__restrict__ tile_off) {
  __shared__ uint32_t s_w[kOneWaves];
  const int t = (int)threadIdx.x, wave = t >> 6;
  int64_t len = n;
  if (kMode != kInit) {
    if (!S->found || (kMode == kRefit && !S->refit_ok)) return;  // (uniform)
    len = S->R;
  }
  const int32_t tiles = (int32_t)((len + kCpTile - 1) / kCpTile);
  uint32_t carry = 0u;
  for (int32_t b = 0; b < tiles; b += kOneBlock) {  // uniform
    const int32_t i = b + t;
    const uint32_t v = i < tiles ? (uint32_t)tile_cnt[i] : 0u;
    const uint32_t incl = wave_incl_scan_u32(v);
    if ((t & 63) == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < kOneWaves; w++) {
      const uint32_t c = s_w[w];
      before += w < wave ? c : 0u;
      total += c;
    }
    __syncthreads();
    if (i < tiles) tile_off[i] = (int32_t)(carry + before + incl - v);
    carry += total;
  }
  if (t != 0) return;
  if (kMode == kInit) {
    const int32_t R = n - (int32_t)carry;
    S->R = R;
    S->run = R >= 3 ? 1 : 0;
  } else if (kMode == kHyp) {
    S->total[0] = (int32_t)carry;
    if (refine) S->cand_size = (int32_t)carry;
  } else {
    S->total[1] = (int32_t)carry;
    S->use = (int32_t)carry >= S->best_count ? 1 : 0;
  }
}

// kToFirst: the live ids of [0, n) and their records -> A_0.  kToCand: the inliers of the hypothesis's plane -> the
// candidate list.  kToNext: the inliers of the kept plane -> ids behind the earlier rounds' and their labels; the rest ->
// A_{r+1}.  A == nullptr: entry i is id i.
template <int kMode>
__global__ __launch_bounds__(kCpBlock) void planes_scatter_kernel(const PlaneState *__restrict__ S, int32_t n, int32_t round,
                                                                  const int32_t *__restrict__ A, const float4 *__restrict__ P,
                                                                  const float4 *__restrict__ N, float max_dist,
                                                                  float min_normal_cos, const int32_t *__restrict__ tile_off0,
                                                                  const int32_t *__restrict__ tile_off1,
                                                                  int32_t *__restrict__ A_out, float4 *__restrict__ P_out,
                                                                  float4 *__restrict__ N_out, int32_t *__restrict__ list,
                                                                  int32_t *__restrict__ labels) {
  __shared__ uint32_t s_w[kCpBlock / 64];
  const int t = (int)threadIdx.x, wave = t >> 6;
  int64_t len = n;
  float pl[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const int32_t *tile_off = tile_off0;
  int32_t list_at = 0;
  if (kMode != kToFirst) {
    if (!S->found) return;  // (uniform)
    len = S->R;
    const int use = kMode == kToNext ? S->use : 0;
    tile_off = use ? tile_off1 : tile_off0;
#pragma unroll
    for (int k = 0; k < 4; k++) pl[k] = S->plane[use][k];
    if (kMode == kToNext) list_at = S->off;
  }
  const int64_t base = (int64_t)blockIdx.x * kCpTile;
  if (base >= len) return;  // (uniform)
  uint32_t gone = (uint32_t)tile_off[blockIdx.x];  // entries that left before this stretch
#pragma unroll 1
  for (int j = 0; j < kCpIters; j++) {
    const int64_t i = base + j * kCpBlock + t;
    const bool valid = i < len;
    const bool leaves = valid && planes_leaves<kMode == kToFirst>(P, N, i, pl, max_dist, min_normal_cos);
    const uint32_t incl = wave_incl_scan_u32(leaves ? 1u : 0u);
    if ((t & 63) == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < kCpBlock / 64; w++) {
      const uint32_t c = s_w[w];
      before += w < wave ? c : 0u;
      total += c;
    }
    __syncthreads();
    const uint32_t pos = gone + before + incl - (leaves ? 1u : 0u);  // entries before i that leave
    if (valid) {
      const int32_t id = A ? A[i] : (int32_t)i;
      if (leaves) {
        if (kMode != kToFirst) list[(int64_t)list_at + pos] = id;
        if (kMode == kToNext) labels[id] = round;
      } else if (kMode != kToCand) {
        const int64_t o = i - (int64_t)pos;
        A_out[o] = id;
        P_out[o] = P[i];
        if (N) N_out[o] = N[i];
      }
    }
    gone += total;
  }
}

__global__ __launch_bounds__(64) void planes_refit_kernel(PlaneState *__restrict__ S, const double *__restrict__ centroid,
                                                          const double *__restrict__ eig, const double *__restrict__ axes,
                                                          PlaneAxis ax) {
  if (threadIdx.x != 0 || !S->found) return;
  float pl[4];
  const double c[3] = {centroid[0], centroid[1], centroid[2]}, a2[3] = {axes[6], axes[7], axes[8]};
  const bool ok = plane_refit(c, a2, eig[0], ax, pl);
  S->refit_ok = ok ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 4; k++) S->plane[1][k] = pl[k];
}

__global__ __launch_bounds__(64) void planes_round_end_kernel(PlaneState *__restrict__ S, int32_t round,
                                                              int32_t *__restrict__ d_n_planes, float *__restrict__ planes,
                                                              int32_t *__restrict__ sizes, int32_t *__restrict__ refined,
                                                              int32_t *__restrict__ best) {
  if (threadIdx.x != 0) return;
  const bool found = S->found != 0;
  const int use = found ? S->use : 0;
  const int32_t size = found ? S->total[use] : 0;
#pragma unroll
  for (int k = 0; k < 4; k++) planes[4 * (int64_t)round + k] = found ? S->plane[use][k] : 0.0f;
  sizes[round] = size;
  refined[round] = use;
  best[round] = found ? S->best : -1;
  if (found) *d_n_planes = round + 1;
  const int32_t R = S->R - size;
  S->off += size;
  S->R = R;
  S->run = found && R >= 3 ? 1 : 0;
  S->found = 0;
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kPlanesMaxRows = 0x7fffffff;
constexpr int32_t kPlanesMaxPlanes = 256;

pcgx_status planes_check(const char *fn, const pcgx_kdtree *t, const void *samples, int64_t n_hyp, int32_t max_planes,
                         float max_dist, int64_t min_inliers, const float *axis, float min_axis_cos, const void *normals,
                         float min_normal_cos) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (n_hyp < 0) return fail(PCGX_E_INVALID, "%s: negative number of hypotheses", fn);
  if (max_planes < 1 || max_planes > kPlanesMaxPlanes)
    return fail(PCGX_E_INVALID, "%s: max_planes must be in [1, %d]", fn, kPlanesMaxPlanes);
  if (!(max_dist > 0.0f) || !(max_dist < __builtin_inff()))
    return fail(PCGX_E_INVALID, "%s: max_dist must be finite and > 0", fn);
  if (min_inliers < 0) return fail(PCGX_E_INVALID, "%s: negative min_inliers", fn);
  if (axis) {
    if (!plane_point_live(axis[0], axis[1], axis[2]) || (axis[0] == 0.0f && axis[1] == 0.0f && axis[2] == 0.0f))
      return fail(PCGX_E_INVALID, "%s: the axis must be finite and not zero", fn);
    if (!(min_axis_cos >= 0.0f) || !(min_axis_cos <= 1.0f))
      return fail(PCGX_E_INVALID, "%s: min_axis_cos must be in [0, 1]", fn);
  }
  if (normals && (!(min_normal_cos >= 0.0f) || !(min_normal_cos <= 1.0f)))
    return fail(PCGX_E_INVALID, "%s: min_normal_cos must be in [0, 1]", fn);
  if (n_hyp > 0 && !samples) return fail(PCGX_E_INVALID, "%s: NULL samples", fn);
  if (n_hyp > kPlanesMaxRows / max_planes)
    return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 hypotheses over all rounds", fn);
  if (t->n > kPlanesMaxRows) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points", fn);
  return PCGX_OK;
}

// PCGX_PLANES_SPLIT=<n>: the number of chunks of the points, forced (tests of the merge, measurements).  Read per call.
int32_t planes_split(int64_t n_hyp, int64_t n) {
  const char *e = getenv("PCGX_PLANES_SPLIT");
  if (e && *e) {
    const long v = atol(e);
    if (v > 0) return (int32_t)(v < kPlMaxSplit ? v : kPlMaxSplit);
  }
  const int64_t tiles = (n_hyp + kPlTile - 1) / kPlTile;
  int64_t s = (kPlTargetWaves + tiles - 1) / tiles;
  const int64_t cap = n / kPlMinChunk;
  if (s > cap) s = cap;
  if (s > kPlMaxSplit) s = kPlMaxSplit;
  return (int32_t)(s < 1 ? 1 : s);
}

}  // namespace

extern "C" int32_t pcgx_planes_tile(void) { return kPlTile; }

extern "C" pcgx_status pcgx_kdtree_planes_dev(const pcgx_kdtree *t, const uint32_t *d_samples, int64_t n_hyp,
                                              int32_t max_planes, float max_dist, int64_t min_inliers, const float *axis,
                                              float min_axis_cos, const float *d_normals, float min_normal_cos,
                                              int32_t refine, int32_t *d_n_planes, float *d_planes, int32_t *d_sizes,
                                              int32_t *d_refined, int32_t *d_best, int32_t *d_labels, int32_t *d_ids,
                                              int32_t *d_status, int32_t *d_counts, float *d_hyp_planes, void *stream) {
  PCGX_API_LOCK();
  const char *fn = "pcgx_kdtree_planes_dev";
  PCGX_TRY(planes_check(fn, t, d_samples, n_hyp, max_planes, max_dist, min_inliers, axis, min_axis_cos, d_normals,
                        min_normal_cos));
  const int64_t n = t->n;
  if (!d_n_planes || !d_planes || !d_sizes || !d_refined || !d_best || (n > 0 && !d_labels))
    return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  const int64_t rows = n_hyp * max_planes;
  if (n == 0 || n_hyp == 0) {
    int64_t most = n > rows ? n : rows;
    if (most < max_planes) most = max_planes;
    hipLaunchKernelGGL(planes_empty_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, st, (int32_t)n, rows,
                       max_planes, d_n_planes, d_planes, d_sizes, d_refined, d_best, d_labels, d_ids, d_status, d_counts,
                       d_hyp_planes);
    PCGX_HIP_TRY(hipGetLastError());
    return PCGX_OK;
  }
  Arena &ar = ctx().arena;
  PCGX_TRY(ar.begin(st));
  const uint32_t *inv = nullptr;
  PCGX_TRY(range_inverse_map(t, &inv, st));
  const int32_t ni = (int32_t)n;
  const size_t N = (size_t)n;
  const unsigned tiles = (unsigned)((n + kCpTile - 1) / kCpTile);
  const bool with_normals = d_normals != nullptr;
  // the lists and records of two rounds in turn (round r reads [r & 1], writes the other); the records by id, which
  // only the first compaction reads, lie where round 0 writes
  int32_t *A[2] = {nullptr, nullptr}, *cand = nullptr, *tile_cnt = nullptr, *tile_off[2] = {nullptr, nullptr};
  float4 *P[2] = {nullptr, nullptr}, *Nr[2] = {nullptr, nullptr};
  PlaneState *S = nullptr;
  double *gs = nullptr;  // centroid [3], eig [3], axes [9]
  uint8_t *d_deleted = nullptr;
  for (int k = 0; k < 2; k++) {
    PCGX_TRY(ar.alloc_n(N, &A[k]));
    PCGX_TRY(ar.alloc_n(N, &P[k]));
    if (with_normals) PCGX_TRY(ar.alloc_n(N, &Nr[k]));
    PCGX_TRY(ar.alloc_n((size_t)tiles, &tile_off[k]));
  }
  PCGX_TRY(ar.alloc_n((size_t)tiles, &tile_cnt));
  if (refine) PCGX_TRY(ar.alloc_n(N, &cand));
  PCGX_TRY(ar.alloc_n(1, &S));
  PCGX_TRY(ar.alloc_n(15, &gs));
  if (!d_ids) PCGX_TRY(ar.alloc_n(N, &d_ids));
  // an optional per-hypothesis output that is not wanted: one round's rows, used by every round in turn
  const int64_t st_stride = d_status ? n_hyp : 0, cn_stride = d_counts ? n_hyp : 0, hp_stride = d_hyp_planes ? n_hyp : 0;
  if (!d_status) PCGX_TRY(ar.alloc_n((size_t)n_hyp, &d_status));
  if (!d_counts) PCGX_TRY(ar.alloc_n((size_t)n_hyp, &d_counts));
  if (!d_hyp_planes) PCGX_TRY(ar.alloc_n((size_t)n_hyp * 4, &d_hyp_planes));
  {
    pcgx_kdtree *tm = const_cast<pcgx_kdtree *>(t);
    std::lock_guard<std::mutex> lock(tm->mu);
    if (t->n_deleted > 0 && (int64_t)t->deleted.size() == n) {
      PCGX_TRY(ar.alloc_n(N, &d_deleted));
      PCGX_TRY(staged_upload(d_deleted, t->deleted.data(), N, st));
      PCGX_HIP_TRY(hipStreamSynchronize(st));  // (the bytes are the handle's: read before the lock is given up)
    }
  }
  const PlaneAxis ax = plane_axis(axis, min_axis_cos);
  PCGX_HIP_TRY(hipMemsetAsync(S, 0, sizeof(PlaneState), st));
  PCGX_HIP_TRY(hipMemsetAsync(d_n_planes, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(planes_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t->d_nodes, inv, ni,
                     (const uint8_t *)d_deleted, d_normals, P[1], Nr[1], d_labels, d_ids);
  hipLaunchKernelGGL(planes_tile_count_kernel<kInit>, dim3(tiles), dim3(kCpBlock), 0, st, (const PlaneState *)S, ni,
                     (const float4 *)P[1], (const float4 *)Nr[1], max_dist, min_normal_cos, tile_cnt);
  hipLaunchKernelGGL(planes_scan_kernel<kInit>, dim3(1), dim3(kOneBlock), 0, st, S, ni, refine, (const int32_t *)tile_cnt,
                     tile_off[0]);
  hipLaunchKernelGGL(planes_scatter_kernel<kToFirst>, dim3(tiles), dim3(kCpBlock), 0, st, (const PlaneState *)S, ni, 0,
                     (const int32_t *)nullptr, (const float4 *)P[1], (const float4 *)Nr[1], max_dist, min_normal_cos,
                     (const int32_t *)tile_off[0], (const int32_t *)tile_off[1], A[0], P[0], Nr[0], (int32_t *)nullptr,
                     (int32_t *)nullptr);
  const int32_t split = planes_split(n_hyp, n);
  int64_t chunk = (n + split - 1) / split;
  if (chunk < 1) chunk = 1;
  const dim3 count_grid((unsigned)((n_hyp + kPlTile - 1) / kPlTile), (unsigned)((n + chunk - 1) / chunk));
  const unsigned fit_blocks = (unsigned)((n_hyp + 255) / 256);
  for (int32_t r = 0; r < max_planes; r++) {
    const int in = r & 1, out = in ^ 1;
    int32_t *status = d_status + st_stride * r, *counts = d_counts + cn_stride * r;
    float *hyp = d_hyp_planes + 4 * hp_stride * r;
    const float4 *Pi = P[in], *Ni = Nr[in];
    hipLaunchKernelGGL(planes_fit_kernel, dim3(fit_blocks), dim3(256), 0, st, (const PlaneState *)S, Pi,
                       d_samples + 3 * n_hyp * r, n_hyp, ax, status, counts, hyp);
    if (with_normals)
      hipLaunchKernelGGL(planes_count_kernel<true>, count_grid, dim3(kPlBlock), 0, st, (const PlaneState *)S, Pi, Ni, n_hyp,
                         (const int32_t *)status, (const float *)hyp, max_dist, min_normal_cos, (int32_t)chunk, counts);
    else
      hipLaunchKernelGGL(planes_count_kernel<false>, count_grid, dim3(kPlBlock), 0, st, (const PlaneState *)S, Pi, Ni, n_hyp,
                         (const int32_t *)status, (const float *)hyp, max_dist, min_normal_cos, (int32_t)chunk, counts);
    hipLaunchKernelGGL(planes_select_kernel, dim3(1), dim3(kOneBlock), 0, st, S, n_hyp, (const int32_t *)status,
                       (const int32_t *)counts, (const float *)hyp, min_inliers);
    hipLaunchKernelGGL(planes_tile_count_kernel<kHyp>, dim3(tiles), dim3(kCpBlock), 0, st, (const PlaneState *)S, ni, Pi, Ni,
                       max_dist, min_normal_cos, tile_cnt);
    hipLaunchKernelGGL(planes_scan_kernel<kHyp>, dim3(1), dim3(kOneBlock), 0, st, S, ni, refine, (const int32_t *)tile_cnt,
                       tile_off[0]);
    if (refine) {
      hipLaunchKernelGGL(planes_scatter_kernel<kToCand>, dim3(tiles), dim3(kCpBlock), 0, st, (const PlaneState *)S, ni, r,
                         (const int32_t *)A[in], Pi, Ni, max_dist, min_normal_cos, (const int32_t *)tile_off[0],
                         (const int32_t *)tile_off[1], (int32_t *)nullptr, (float4 *)nullptr, (float4 *)nullptr, cand,
                         (int32_t *)nullptr);
      const Arena::Mark mark = ar.mark();
      PCGX_TRY(group_frames_enqueue(t, cand, n, &S->cand_size, 1, gs, gs + 3, gs + 6, st));
      ar.rewind(mark);
      hipLaunchKernelGGL(planes_refit_kernel, dim3(1), dim3(64), 0, st, S, (const double *)gs, (const double *)(gs + 3),
                         (const double *)(gs + 6), ax);
      hipLaunchKernelGGL(planes_tile_count_kernel<kRefit>, dim3(tiles), dim3(kCpBlock), 0, st, (const PlaneState *)S, ni, Pi,
                         Ni, max_dist, min_normal_cos, tile_cnt);
      hipLaunchKernelGGL(planes_scan_kernel<kRefit>, dim3(1), dim3(kOneBlock), 0, st, S, ni, refine,
                         (const int32_t *)tile_cnt, tile_off[1]);
    }
    hipLaunchKernelGGL(planes_scatter_kernel<kToNext>, dim3(tiles), dim3(kCpBlock), 0, st, (const PlaneState *)S, ni, r,
                       (const int32_t *)A[in], Pi, Ni, max_dist, min_normal_cos, (const int32_t *)tile_off[0],
                       (const int32_t *)tile_off[1], A[out], P[out], Nr[out], d_ids, d_labels);
    hipLaunchKernelGGL(planes_round_end_kernel, dim3(1), dim3(64), 0, st, S, r, d_n_planes, d_planes, d_sizes, d_refined,
                       d_best);
  }
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_kdtree_planes(const pcgx_kdtree *t, const uint32_t *samples, int64_t n_hyp, int32_t max_planes,
                                          float max_dist, int64_t min_inliers, const float *axis, float min_axis_cos,
                                          const float *normals, float min_normal_cos, int32_t refine, int64_t *n_planes,
                                          float *planes, int64_t *sizes, int32_t *refined, int64_t *best, int64_t *labels,
                                          int64_t *ids, int32_t *status, int64_t *counts, float *hyp_planes) {
  PCGX_API_CALL();
  const char *fn = "pcgx_kdtree_planes";
  PCGX_TRY(planes_check(fn, t, samples, n_hyp, max_planes, max_dist, min_inliers, axis, min_axis_cos, normals,
                        min_normal_cos));
  const int64_t n = t->n;
  if (!n_planes || !planes || !sizes || !refined || !best || (n > 0 && !labels))
    return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  const size_t N = (size_t)n, M = (size_t)max_planes, H = (size_t)(n_hyp * max_planes);
  // one block of int32 words: n_planes, sizes, refined, best, labels, ids; then the per-hypothesis rows
  const size_t words = 1 + 3 * M + 2 * N;
  int32_t *d_out = nullptr, *d_status = nullptr, *d_counts = nullptr;
  float *d_planes = nullptr, *d_hyp = nullptr, *d_normals = nullptr;
  uint32_t *d_samples = nullptr;
  PCGX_TRY(ha.alloc_n(words, &d_out));
  PCGX_TRY(ha.alloc_n(4 * M, &d_planes));
  if (status && H) PCGX_TRY(ha.alloc_n(H, &d_status));
  if (counts && H) PCGX_TRY(ha.alloc_n(H, &d_counts));
  if (hyp_planes && H) PCGX_TRY(ha.alloc_n(4 * H, &d_hyp));
  if (H) {
    PCGX_TRY(ha.alloc_n(3 * H, &d_samples));
    PCGX_TRY(staged_upload(d_samples, samples, 12 * H, st));
  }
  if (normals && N) {
    PCGX_TRY(ha.alloc_n(3 * N, &d_normals));
    PCGX_TRY(staged_upload(d_normals, normals, 12 * N, st));
  }
  int32_t *d_sizes = d_out + 1, *d_refined = d_sizes + M, *d_best = d_refined + M, *d_labels = d_best + M,
          *d_ids = d_labels + N;
  // (normals of an empty tree: the pointer says that they are given, nothing reads it)
  PCGX_TRY(pcgx_kdtree_planes_dev(t, d_samples, n_hyp, max_planes, max_dist, min_inliers, axis, min_axis_cos,
                                  normals && N ? d_normals : nullptr, min_normal_cos, refine, d_out, d_planes, d_sizes,
                                  d_refined, d_best, d_labels, d_ids, d_status, d_counts, d_hyp, st));
  RawVector<int32_t> r(words);
  PCGX_TRY(staged_download(r.data(), d_out, words * 4, st));
  PCGX_TRY(staged_download(planes, d_planes, 16 * M, st));
  *n_planes = r[0];
  for (size_t k = 0; k < M; k++) {
    sizes[k] = r[1 + k];
    refined[k] = r[1 + M + k];
    best[k] = r[1 + 2 * M + k];
  }
  for (size_t i = 0; i < N; i++) labels[i] = r[1 + 3 * M + i];
  if (ids)
    for (size_t i = 0; i < N; i++) ids[i] = r[1 + 3 * M + N + i];
  if (status && H) PCGX_TRY(staged_download(status, d_status, H * 4, st));
  if (hyp_planes && H) PCGX_TRY(staged_download(hyp_planes, d_hyp, H * 16, st));
  if (counts && H) {
    RawVector<int32_t> c(H);
    PCGX_TRY(staged_download(c.data(), d_counts, H * 4, st));
    for (size_t i = 0; i < H; i++) counts[i] = c[i];
  }
  return PCGX_OK;
}
