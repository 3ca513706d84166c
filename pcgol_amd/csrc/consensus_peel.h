// consensus_peel.h -- the round machinery of the sample-consensus segmentations (planes.hip, shapes.hip): the model most
// of the cloud agrees on over the caller's samples, its inliers taken out ("peeled"), then the next one.  All rounds are
// enqueued up front; a round reads from device words (PeelState) how many points are left and whether an earlier round
// failed, and every kernel of a round that does not run returns at once.  No kernel waits on another workgroup.
//
// A round works on the points that are left, A_r, as a list of ids in ascending order with their point and normal
// records compacted beside it, in two buffers used in turn.  A file brings its hypotheses (a fit and a count kernel), its
// refit, and a model:
//   kRec, kMinSample   floats of a record (a plane's four, a shape's eight), points of a minimal sample
//   Test               the call's constants of the inlier test, a kernel argument
//   Rec, load()        a record as the compaction holds it (with what load() derives from it once a workgroup)
//   inlier()           is the point p, entry i of the list, an inlier of the record?  N is null without normals
// and this header the rest:
//   peel_gather_kernel      once: a lane per id, the point (and its normal) into records by id, NaN where the point is
//                           not live; the by-id "still left" flag where asked for; labels and ids to -1.
//   peel_select_kernel      ONE workgroup: the first best (a max over (count + 1) << 32 | ~h), found or not.
//   peel_tile_count_kernel  the ordered compaction, three kernels (many workgroups, one for the tile offsets): how many
//   peel_scan_kernel        entries of each tile of 1024 leave (init: are not live; else: are inliers of the round's
//   peel_scatter_kernel     record), the exclusive scan of that, and the scatter: those that leave to the inlier list in
//                           order, those that stay to the next round's list and records in order.
//   peel_round_end_kernel   one lane: the round's row of the outputs, and the state of the next round.
//   peel_empty_kernel       n_hyp == 0 or Len() == 0: every row of every output.
// and the host side of a call: the checks both share, the buffers, the first list, the rounds, the host form.
#pragma once
#include <stdlib.h>

#include <mutex>

#include "plane_terms.h"
#include "range_walk.h"

namespace pcgx {

constexpr int kPeelBlock = 64;             // a count kernel: one wave per workgroup
constexpr int kPeelTile = 2 * kPeelBlock;  // ... and its hypotheses: lane l has tile * 128 + l and + 64 + l
constexpr int kPeelTargetWaves = 65536;    // the split makes about this many waves (as pose.hip)
constexpr int kPeelMinChunk = 256;         // ... but leaves a chunk at least this many points
constexpr int kPeelMaxSplit = 65535;       // gridDim.y
constexpr int kCpBlock = 256, kCpIters = 4;
constexpr int kCpTile = kCpBlock * kCpIters;  // entries per workgroup of the compaction
constexpr int kOneBlock = 1024;               // the one-workgroup kernels
constexpr int kOneWaves = kOneBlock / 64;
constexpr int64_t kPeelMaxRows = 0x7fffffff;
constexpr int32_t kPeelMaxRounds = 256;
constexpr int32_t kPeelNotRun = -1, kPeelOk = 0;  // every model's status codes begin so

// The device words the rounds hand on.
template <int kRec>
struct PeelState {
  int32_t run;         // this round runs
  int32_t R;           // |A_r|
  int32_t off;         // inliers of the earlier rounds: where this round's go in ids
  int32_t found;       // the round found a model (select)
  int32_t best, best_count;
  int32_t cand_size;   // the best hypothesis's inliers, 0 when nothing is refitted (planes: the word group geometry reads)
  int32_t refit_ok;    // rec[1] is a refitted record
  int32_t use;         // the kept record: 0 the hypothesis's, 1 the refitted one
  int32_t total[2];    // the inliers of rec[0] and rec[1]
  int32_t pad;
  float rec[2][kRec];
};

enum { kInit = 0, kHyp = 1, kRefit = 2 };         // what a tile count / scan is for
enum { kToFirst = 0, kToCand = 1, kToNext = 2 };  // ... and a scatter

// (static: each source file that includes this launches its own copy)
static __global__ __launch_bounds__(256) void peel_gather_kernel(const float4 *__restrict__ nodes,
                                                                 const uint32_t *__restrict__ inv, int32_t n,
                                                                 const uint8_t *__restrict__ deleted,
                                                                 const float *__restrict__ normals, float4 *__restrict__ P,
                                                                 float4 *__restrict__ N, uint8_t *__restrict__ left,
                                                                 int32_t *__restrict__ labels, int32_t *__restrict__ ids) {
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
  if (left) left[i] = live ? (uint8_t)1 : (uint8_t)0;
  labels[i] = -1;
  ids[i] = -1;
}

// n_hyp == 0 or Len() == 0: nothing runs, every row of every output is written
template <int kRec>
__global__ __launch_bounds__(256) void peel_empty_kernel(int32_t n, int64_t rows, int32_t rounds,
                                                         int32_t *__restrict__ d_n_found, float *__restrict__ recs,
                                                         int32_t *__restrict__ sizes, int32_t *__restrict__ refined,
                                                         int32_t *__restrict__ best, int32_t *__restrict__ labels,
                                                         int32_t *__restrict__ ids, int32_t *__restrict__ status,
                                                         int32_t *__restrict__ counts, float *__restrict__ hyp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *d_n_found = 0;
  if (i < n) {
    labels[i] = -1;
    if (ids) ids[i] = -1;
  }
  if (i < rounds) {
#pragma unroll
    for (int k = 0; k < kRec; k++) recs[kRec * i + k] = 0.0f;
    sizes[i] = 0;
    refined[i] = 0;
    best[i] = -1;
  }
  if (i < rows) {
    if (status) status[i] = kPeelNotRun;
    if (counts) counts[i] = 0;
    if (hyp) {
#pragma unroll
      for (int k = 0; k < kRec; k++) hyp[kRec * i + k] = 0.0f;
    }
  }
}

template <class M>
__global__ __launch_bounds__(kOneBlock) void peel_select_kernel(PeelState<M::kRec> *__restrict__ S, int64_t n_hyp,
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
      if (status[h] == kPeelOk) {
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
  const int64_t need = min_inliers > M::kMinSample ? min_inliers : M::kMinSample;
  const bool found = run && key && (int64_t)best_count >= need;
  S->found = found ? 1 : 0;
  S->best = best;
  S->best_count = best_count;
  S->cand_size = 0;
  S->refit_ok = 0;
  S->use = 0;
  S->total[0] = S->total[1] = 0;
#pragma unroll
  for (int k = 0; k < M::kRec; k++) {
    S->rec[0][k] = found ? hyp[M::kRec * (int64_t)best + k] : 0.0f;
    S->rec[1][k] = 0.0f;
  }
}

// ---- the ordered compaction

// does entry i leave the list?  init: it is not live (its record is NaN); else: it is an inlier of rec
template <class M, bool kIsInit>
__device__ __forceinline__ bool peel_leaves(const float4 *__restrict__ P, const float4 *__restrict__ N, int64_t i,
                                            const typename M::Rec &rec, const typename M::Test &T) {
  const float4 p = P[i];
  if (kIsInit) return !(p.x == p.x);
  return M::inlier(rec, T, p, N, i);
}

template <class M, int kMode>
__global__ __launch_bounds__(kCpBlock) void peel_tile_count_kernel(const PeelState<M::kRec> *__restrict__ S, int32_t n,
                                                                   const float4 *__restrict__ P,
                                                                   const float4 *__restrict__ N, typename M::Test T,
                                                                   int32_t *__restrict__ tile_cnt) {
  __shared__ int32_t s_w[kCpBlock / 64];
  int64_t len = n;
  typename M::Rec rec = {};
  if (kMode != kInit) {
    if (!S->found || (kMode == kRefit && !S->refit_ok)) return;  // (uniform)
    len = S->R;
    rec = M::load(S->rec[kMode == kRefit ? 1 : 0], T);
  }
  const int64_t base = (int64_t)blockIdx.x * kCpTile;
  if (base >= len) return;  // (uniform; the scan reads the tiles below len only)
  int32_t c = 0;
#pragma unroll
  for (int j = 0; j < kCpIters; j++) {
    const int64_t i = base + j * kCpBlock + threadIdx.x;
    if (i < len) c += peel_leaves<M, kMode == kInit>(P, N, i, rec, T) ? 1 : 0;
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
template <class M, int kMode>
__global__ __launch_bounds__(kOneBlock) void peel_scan_kernel(PeelState<M::kRec> *__restrict__ S, int32_t n, int32_t refine,
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
    S->run = R >= M::kMinSample ? 1 : 0;
  } else if (kMode == kHyp) {
    S->total[0] = (int32_t)carry;
    if (refine) S->cand_size = (int32_t)carry;
  } else {
    S->total[1] = (int32_t)carry;
    S->use = (int32_t)carry >= S->best_count ? 1 : 0;
  }
}

// kToFirst: the live ids of [0, n) and their records -> A_0.  kToCand: the inliers of the hypothesis's record -> the
// candidate list.  kToNext: the inliers of the kept record -> ids behind the earlier rounds', their labels, their left
// flag (where there is one) cleared; the rest -> A_{r+1}.  A == nullptr: entry i is id i.
template <class M, int kMode>
__global__ __launch_bounds__(kCpBlock) void peel_scatter_kernel(const PeelState<M::kRec> *__restrict__ S, int32_t n,
                                                                int32_t round, const int32_t *__restrict__ A,
                                                                const float4 *__restrict__ P, const float4 *__restrict__ N,
                                                                typename M::Test T, const int32_t *__restrict__ tile_off0,
                                                                const int32_t *__restrict__ tile_off1,
                                                                int32_t *__restrict__ A_out, float4 *__restrict__ P_out,
                                                                float4 *__restrict__ N_out, int32_t *__restrict__ list,
                                                                int32_t *__restrict__ labels, uint8_t *__restrict__ left) {
  __shared__ uint32_t s_w[kCpBlock / 64];
  const int t = (int)threadIdx.x, wave = t >> 6;
  int64_t len = n;
  typename M::Rec rec = {};
  const int32_t *tile_off = tile_off0;
  int32_t list_at = 0;
  if (kMode != kToFirst) {
    if (!S->found) return;  // (uniform)
    len = S->R;
    const int use = kMode == kToNext ? S->use : 0;
    tile_off = use ? tile_off1 : tile_off0;
    rec = M::load(S->rec[use], T);
    if (kMode == kToNext) list_at = S->off;
  }
  const int64_t base = (int64_t)blockIdx.x * kCpTile;
  if (base >= len) return;  // (uniform)
  uint32_t gone = (uint32_t)tile_off[blockIdx.x];  // entries that left before this stretch
#pragma unroll 1
  for (int j = 0; j < kCpIters; j++) {
    const int64_t i = base + j * kCpBlock + t;
    const bool valid = i < len;
    const bool leaves = valid && peel_leaves<M, kMode == kToFirst>(P, N, i, rec, T);
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
        if (kMode == kToNext) {
          labels[id] = round;
          if (left) left[id] = (uint8_t)0;
        }
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

template <class M>
__global__ __launch_bounds__(64) void peel_round_end_kernel(PeelState<M::kRec> *__restrict__ S, int32_t round,
                                                            int32_t *__restrict__ d_n_found, float *__restrict__ recs,
                                                            int32_t *__restrict__ sizes, int32_t *__restrict__ refined,
                                                            int32_t *__restrict__ best) {
  if (threadIdx.x != 0) return;
  const bool found = S->found != 0;
  const int use = found ? S->use : 0;
  const int32_t size = found ? S->total[use] : 0;
#pragma unroll
  for (int k = 0; k < M::kRec; k++) recs[M::kRec * (int64_t)round + k] = found ? S->rec[use][k] : 0.0f;
  sizes[round] = size;
  refined[round] = use;
  best[round] = found ? S->best : -1;
  if (found) *d_n_found = round + 1;
  const int32_t R = S->R - size;
  S->off += size;
  S->R = R;
  S->run = found && R >= M::kMinSample ? 1 : 0;
  S->found = 0;
}

// ---- the host side

// The checks both entry points share, in three parts: a file's own checks stand between them.  `rounds_name`:
// "max_planes" or "max_shapes".
inline pcgx_status peel_check_counts(const char *fn, int64_t n_hyp, const char *rounds_name, int32_t rounds, float max_dist,
                                     int64_t min_inliers) {
  if (n_hyp < 0) return fail(PCGX_E_INVALID, "%s: negative number of hypotheses", fn);
  if (rounds < 1 || rounds > kPeelMaxRounds)
    return fail(PCGX_E_INVALID, "%s: %s must be in [1, %d]", fn, rounds_name, kPeelMaxRounds);
  if (!(max_dist > 0.0f) || !(max_dist < __builtin_inff()))
    return fail(PCGX_E_INVALID, "%s: max_dist must be finite and > 0", fn);
  if (min_inliers < 0) return fail(PCGX_E_INVALID, "%s: negative min_inliers", fn);
  return PCGX_OK;
}

inline pcgx_status peel_check_axis(const char *fn, const float *axis, float min_axis_cos) {
  if (!axis) return PCGX_OK;
  if (!plane_point_live(axis[0], axis[1], axis[2]) || (axis[0] == 0.0f && axis[1] == 0.0f && axis[2] == 0.0f))
    return fail(PCGX_E_INVALID, "%s: the axis must be finite and not zero", fn);
  if (!(min_axis_cos >= 0.0f) || !(min_axis_cos <= 1.0f))
    return fail(PCGX_E_INVALID, "%s: min_axis_cos must be in [0, 1]", fn);
  return PCGX_OK;
}

inline pcgx_status peel_check_sizes(const char *fn, const pcgx_kdtree *t, const void *samples, int64_t n_hyp, int32_t rounds) {
  if (n_hyp > 0 && !samples) return fail(PCGX_E_INVALID, "%s: NULL samples", fn);
  if (n_hyp > kPeelMaxRows / rounds) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 hypotheses over all rounds", fn);
  if (t->n > kPeelMaxRows) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points", fn);
  return PCGX_OK;
}

// The grid of a count kernel (hypothesis tiles x chunks of the points) and the chunk.  The environment variable `env`
// (PCGX_PLANES_SPLIT, PCGX_SHAPES_SPLIT) =<n>: the number of chunks, forced (tests of the merge, measurements).  Read
// per call.
inline int32_t peel_split(const char *env, int64_t n_hyp, int64_t n) {
  const char *e = getenv(env);
  if (e && *e) {
    const long v = atol(e);
    if (v > 0) return (int32_t)(v < kPeelMaxSplit ? v : kPeelMaxSplit);
  }
  const int64_t tiles = (n_hyp + kPeelTile - 1) / kPeelTile;
  int64_t s = (kPeelTargetWaves + tiles - 1) / tiles;
  const int64_t cap = n / kPeelMinChunk;
  if (s > cap) s = cap;
  if (s > kPeelMaxSplit) s = kPeelMaxSplit;
  return (int32_t)(s < 1 ? 1 : s);
}
inline dim3 peel_count_grid(const char *env, int64_t n_hyp, int64_t n, int32_t *chunk) {
  const int32_t split = peel_split(env, n_hyp, n);
  int64_t c = (n + split - 1) / split;
  if (c < 1) c = 1;
  *chunk = (int32_t)c;
  return dim3((unsigned)((n_hyp + kPeelTile - 1) / kPeelTile), (unsigned)((n + c - 1) / c));
}

// A call's outputs, device addresses (ids, status, counts, hyp: null where not wanted).
struct PeelOut {
  int32_t *n_found;
  float *recs;
  int32_t *sizes, *refined, *best, *labels, *ids, *status, *counts;
  float *hyp;
};

template <int kRec>
pcgx_status peel_empty(int64_t n, int64_t rows, int32_t rounds, const PeelOut &o, hipStream_t st) {
  int64_t most = n > rows ? n : rows;
  if (most < rounds) most = rounds;
  hipLaunchKernelGGL(peel_empty_kernel<kRec>, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, st, (int32_t)n, rows, rounds,
                     o.n_found, o.recs, o.sizes, o.refined, o.best, o.labels, o.ids, o.status, o.counts, o.hyp);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

// The lists and records of two rounds in turn (round r reads [r & 1], writes the other) and the rest both files need.
template <int kRec>
struct PeelBuffers {
  int32_t *A[2] = {nullptr, nullptr}, *cand = nullptr, *tile_cnt = nullptr, *tile_off[2] = {nullptr, nullptr};
  float4 *P[2] = {nullptr, nullptr}, *Nr[2] = {nullptr, nullptr};
  PeelState<kRec> *S = nullptr;
  uint8_t *deleted = nullptr;                          // the handle's deleted bytes, null where it has none
  int64_t st_stride = 0, cn_stride = 0, hp_stride = 0;  // rows a round of status / counts / hyp, 0 for a stand-in
  unsigned tiles = 0;
};

// ... from the call's arena; o's ids, status, counts and hyp are given stand-ins where they are null
template <int kRec>
pcgx_status peel_buffers(const pcgx_kdtree *t, Arena &ar, int64_t n_hyp, bool with_normals, bool refine, PeelOut *o,
                         PeelBuffers<kRec> *b, hipStream_t st) {
  const size_t N = (size_t)t->n;
  b->tiles = (unsigned)((t->n + kCpTile - 1) / kCpTile);
  for (int k = 0; k < 2; k++) {
    PCGX_TRY(ar.alloc_n(N, &b->A[k]));
    PCGX_TRY(ar.alloc_n(N, &b->P[k]));
    if (with_normals) PCGX_TRY(ar.alloc_n(N, &b->Nr[k]));
    PCGX_TRY(ar.alloc_n((size_t)b->tiles, &b->tile_off[k]));
  }
  PCGX_TRY(ar.alloc_n((size_t)b->tiles, &b->tile_cnt));
  if (refine) PCGX_TRY(ar.alloc_n(N, &b->cand));
  PCGX_TRY(ar.alloc_n(1, &b->S));
  if (!o->ids) PCGX_TRY(ar.alloc_n(N, &o->ids));
  // an optional per-hypothesis output that is not wanted: one round's rows, used by every round in turn
  b->st_stride = o->status ? n_hyp : 0, b->cn_stride = o->counts ? n_hyp : 0, b->hp_stride = o->hyp ? n_hyp : 0;
  if (!o->status) PCGX_TRY(ar.alloc_n((size_t)n_hyp, &o->status));
  if (!o->counts) PCGX_TRY(ar.alloc_n((size_t)n_hyp, &o->counts));
  if (!o->hyp) PCGX_TRY(ar.alloc_n((size_t)n_hyp * kRec, &o->hyp));
  pcgx_kdtree *tm = const_cast<pcgx_kdtree *>(t);
  std::lock_guard<std::mutex> lock(tm->mu);
  if (t->n_deleted > 0 && (int64_t)t->deleted.size() == t->n) {
    PCGX_TRY(ar.alloc_n(N, &b->deleted));
    PCGX_TRY(staged_upload(b->deleted, t->deleted.data(), N, st));
    PCGX_HIP_TRY(hipStreamSynchronize(st));  // (the bytes are the handle's: read before the lock is given up)
  }
  return PCGX_OK;
}

// the tile count of kMode and its scan into tile_off
template <class M, int kMode>
void peel_count_scan(const PeelBuffers<M::kRec> &b, int32_t n, int32_t refine, const float4 *P, const float4 *N,
                     const typename M::Test &T, int32_t *tile_off, hipStream_t st) {
  const PeelState<M::kRec> *S = b.S;
  const int32_t *tile_cnt = b.tile_cnt;
  hipLaunchKernelGGL((peel_tile_count_kernel<M, kMode>), dim3(b.tiles), dim3(kCpBlock), 0, st, S, n, P, N, T, b.tile_cnt);
  hipLaunchKernelGGL((peel_scan_kernel<M, kMode>), dim3(1), dim3(kOneBlock), 0, st, b.S, n, refine, tile_cnt, tile_off);
}

template <class M, int kMode>
void peel_scatter(const PeelBuffers<M::kRec> &b, int32_t n, int32_t round, const int32_t *A, const float4 *P, const float4 *N,
                  const typename M::Test &T, int32_t *A_out, float4 *P_out, float4 *N_out, int32_t *list, int32_t *labels,
                  uint8_t *left, hipStream_t st) {
  const PeelState<M::kRec> *S = b.S;
  const int32_t *off0 = b.tile_off[0], *off1 = b.tile_off[1];
  hipLaunchKernelGGL((peel_scatter_kernel<M, kMode>), dim3(b.tiles), dim3(kCpBlock), 0, st, S, n, round, A, P, N, T, off0, off1,
                     A_out, P_out, N_out, list, labels, left);
}

// The head of a call: the state and n_found to zero, the records by id (Pid, and Nid where there are normals), and the
// first compaction: the live ids and their records -> A_0.
template <class M>
pcgx_status peel_first(const pcgx_kdtree *t, const uint32_t *inv, const PeelBuffers<M::kRec> &b, const typename M::Test &T,
                       const float *d_normals, float4 *Pid, float4 *Nid, uint8_t *left, const PeelOut &o, hipStream_t st) {
  const int32_t n = (int32_t)t->n;
  PCGX_HIP_TRY(hipMemsetAsync(b.S, 0, sizeof(PeelState<M::kRec>), st));
  PCGX_HIP_TRY(hipMemsetAsync(o.n_found, 0, sizeof(int32_t), st));
  const uint8_t *deleted = b.deleted;
  hipLaunchKernelGGL(peel_gather_kernel, dim3((unsigned)((t->n + 255) / 256)), dim3(256), 0, st, t->d_nodes, inv, n, deleted,
                     d_normals, Pid, Nid, left, o.labels, o.ids);
  peel_count_scan<M, kInit>(b, n, 0, Pid, Nid, T, b.tile_off[0], st);
  peel_scatter<M, kToFirst>(b, n, 0, nullptr, Pid, Nid, T, b.A[0], b.P[0], b.Nr[0], nullptr, nullptr, nullptr, st);
  return PCGX_OK;
}

// what a round's own kernels are given: its list and records, its rows of the per-hypothesis outputs
struct PeelRound {
  int32_t r;
  const int32_t *A;
  const float4 *P, *N;
  int32_t *status, *counts;
  float *hyp;
};

// Every round, enqueued: fit(round) launches the file's fit and count kernels; refit(round) -> pcgx_status what makes
// rec[1] and refit_ok from the candidate list b.cand (its size in S->cand_size).
template <class M, class Fit, class Refit>
pcgx_status peel_rounds(const PeelBuffers<M::kRec> &b, int32_t n, int64_t n_hyp, int32_t rounds, int64_t min_inliers,
                        int32_t refine, const typename M::Test &T, uint8_t *left, const PeelOut &o, hipStream_t st, Fit fit,
                        Refit refit) {
  for (int32_t r = 0; r < rounds; r++) {
    const int in = r & 1, out = in ^ 1;
    const PeelRound q{r, b.A[in], b.P[in], b.Nr[in], o.status + b.st_stride * r, o.counts + b.cn_stride * r,
                      o.hyp + M::kRec * b.hp_stride * r};
    const int32_t *status = q.status, *counts = q.counts;
    const float *hyp = q.hyp;
    fit(q);
    hipLaunchKernelGGL(peel_select_kernel<M>, dim3(1), dim3(kOneBlock), 0, st, b.S, n_hyp, status, counts, hyp, min_inliers);
    peel_count_scan<M, kHyp>(b, n, refine, q.P, q.N, T, b.tile_off[0], st);
    if (refine) {
      peel_scatter<M, kToCand>(b, n, r, q.A, q.P, q.N, T, nullptr, nullptr, nullptr, b.cand, nullptr, nullptr, st);
      PCGX_TRY(refit(q));
      peel_count_scan<M, kRefit>(b, n, refine, q.P, q.N, T, b.tile_off[1], st);
    }
    peel_scatter<M, kToNext>(b, n, r, q.A, q.P, q.N, T, b.A[out], b.P[out], b.Nr[out], o.ids, o.labels, left, st);
    hipLaunchKernelGGL(peel_round_end_kernel<M>, dim3(1), dim3(64), 0, st, b.S, r, o.n_found, o.recs, o.sizes, o.refined,
                       o.best);
  }
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

// The host form: samples (sample_words a hypothesis) and normals up, dev(d_samples, d_normals, outputs, stream) -- the
// file's device form -- on the library's stream, the outputs (records of kRec floats) down and widened.
template <int kRec, class Dev>
pcgx_status peel_host(int64_t n, int sample_words, const uint32_t *samples, int64_t n_hyp, int32_t rounds,
                      const float *normals, int64_t *n_found, float *recs, int64_t *sizes, int32_t *refined, int64_t *best,
                      int64_t *labels, int64_t *ids, int32_t *status, int64_t *counts, float *hyp, Dev dev) {
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  const size_t N = (size_t)n, M = (size_t)rounds, H = (size_t)(n_hyp * rounds), W = (size_t)sample_words;
  // one block of int32 words: n_found, sizes, refined, best, labels, ids; then the per-hypothesis rows
  const size_t words = 1 + 3 * M + 2 * N;
  int32_t *d_out = nullptr;
  PeelOut d{};
  float *d_normals = nullptr;
  uint32_t *d_samples = nullptr;
  PCGX_TRY(ha.alloc_n(words, &d_out));
  PCGX_TRY(ha.alloc_n(kRec * M, &d.recs));
  if (status && H) PCGX_TRY(ha.alloc_n(H, &d.status));
  if (counts && H) PCGX_TRY(ha.alloc_n(H, &d.counts));
  if (hyp && H) PCGX_TRY(ha.alloc_n(kRec * H, &d.hyp));
  if (H) {
    PCGX_TRY(ha.alloc_n(W * H, &d_samples));
    PCGX_TRY(staged_upload(d_samples, samples, 4 * W * H, st));
  }
  // (normals of an empty tree: nothing is uploaded, and the device form is told that there are none)
  if (normals && N) {
    PCGX_TRY(ha.alloc_n(3 * N, &d_normals));
    PCGX_TRY(staged_upload(d_normals, normals, 12 * N, st));
  }
  d.n_found = d_out, d.sizes = d_out + 1, d.refined = d.sizes + M, d.best = d.refined + M, d.labels = d.best + M;
  d.ids = d.labels + N;
  PCGX_TRY(dev(d_samples, d_normals, d, st));
  RawVector<int32_t> r(words);
  PCGX_TRY(staged_download(r.data(), d_out, words * 4, st));
  PCGX_TRY(staged_download(recs, d.recs, 4 * kRec * M, st));
  *n_found = r[0];
  for (size_t k = 0; k < M; k++) {
    sizes[k] = r[1 + k];
    refined[k] = r[1 + M + k];
    best[k] = r[1 + 2 * M + k];
  }
  for (size_t i = 0; i < N; i++) labels[i] = r[1 + 3 * M + i];
  if (ids)
    for (size_t i = 0; i < N; i++) ids[i] = r[1 + 3 * M + N + i];
  if (status && H) PCGX_TRY(staged_download(status, d.status, H * 4, st));
  if (hyp && H) PCGX_TRY(staged_download(hyp, d.hyp, H * 4 * kRec, st));
  if (counts && H) {
    RawVector<int32_t> c(H);
    PCGX_TRY(staged_download(c.data(), d.counts, H * 4, st));
    for (size_t i = 0; i < H; i++) counts[i] = c[i];
  }
  return PCGX_OK;
}

}  // namespace pcgx
