// shapes.hip -- cylinder and sphere segmentation: the shape most of the cloud agrees on, by sample consensus over
// hypotheses made from two oriented points (Schnabel et al. 2007), the second drawn from the first's radius
// neighbourhood; its inliers taken out, then the next one (extension: no reference parity; include/pcgx.h, "shapes").
// The contract and the round machinery are planes.hip's: the caller draws every random word, every round is enqueued
// up front and reads from device words (ShapeState) how many points are left and whether an earlier round failed, every
// kernel of a round that does not run returns at once, and no kernel waits on another workgroup.
//
//   shapes_gather_kernel      once: a lane per id, the point and its normal into records by id (32 bytes a point), NaN
//                             where the point is not live; the by-id "still left" flag; labels and ids to -1.
//   shapes_partner_kernel     <kSrc> a lane per hypothesis, one-wave workgroups: the seed's radius neighbourhood through
//                             radius_visit (radius_visit.h) on the grid, the tree walk and the patched walk; take keeps
//                             the minimum of (mix << 32) | id over the candidates that are left.  A fat row is shared
//                             by the wave, the partial minima reduced over the lanes into the owner.  No list is stored:
//                             the choice is a property of the set.  Not launched with sample_radius == 0.
//   shapes_fit_kernel         a lane per hypothesis: shape_terms.h's shape_hypothesis -> status and record, count 0.
//   shapes_count_kernel       <kind, normal test> the hot one, hypotheses x points: planes_count_kernel's shape.  One wave
//                             per workgroup, TWO hypotheses per lane, their numbers and lo2 / hi2 as packed float32 pairs
//                             (each half rounded on its own), the point and normal records wave-uniform through scalar
//                             loads, blockIdx.y over chunks of the list, an integer atomicAdd per lane at the end.  No LDS.
//   shapes_select_kernel      ONE workgroup: the first best, found or not.
//   shapes_tile_count_kernel  the ordered compaction (tile count, scan, scatter), planes.hip's logic with the shape's
//   shapes_scan_kernel        inlier test as what leaves; the scatter to the next round also clears the left flag of
//   shapes_scatter_kernel     the inliers.
//   shapes_sums_kernel        the refit's sums over the candidate inlier list: a tile of 1024 a workgroup, a lane's four
//                             entries in order, a fixed shuffle tree, the four waves in order -> 13 doubles a tile.
//   shapes_refit_kernel       one wave adds the tile partials in tile order, one lane solves (shape_terms.h's shape_refit).
//   shapes_round_end_kernel   one lane: the round's row of the outputs, and the state of the next round.
// These are shapes.hip's own kernels and not planes.hip's: what leaves a list (the inlier test), the record a round
// hands on (eight numbers, not four) and the left flag differ, and planes.hip's kernels and their names are pinned by
// its resource test.  Integer atomics only: the same input gives the same bits on every call, whatever the split.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "radius_visit.h"
#include "shape_terms.h"

namespace pcgx {

constexpr int kShBlock = kRangeWalkBlock;  // one wave per workgroup (the walks' LDS frame stacks are [level][64])
constexpr int kShTile = 2 * kShBlock;      // hypotheses per workgroup of the count: lane l has tile * 128 + l and + 64 + l
constexpr int kShTargetWaves = 65536;      // the split makes about this many waves (as planes.hip)
constexpr int kShMinChunk = 256;           // ... but leaves a chunk at least this many points
constexpr int kShMaxSplit = 65535;         // gridDim.y
constexpr int kScBlock = 256, kScIters = 4;
constexpr int kScTile = kScBlock * kScIters;  // entries per workgroup of the compaction and of the sums
constexpr int kShOneBlock = 1024;             // the one-workgroup kernels
constexpr int kShOneWaves = kShOneBlock / 64;
static_assert(kShBlock == 64, "one wave per workgroup");

typedef float shape_f2 __attribute__((ext_vector_type(2)));

// The device words the rounds hand on.
struct ShapeState {
  int32_t run;         // this round runs
  int32_t R;           // |A_r|
  int32_t off;         // inliers of the earlier rounds: where this round's go in ids
  int32_t found;       // the round found a shape (select)
  int32_t best, best_count;
  int32_t cand_size;   // the best hypothesis's inliers, 0 when nothing is refitted
  int32_t refit_ok;    // rec[1] is a refitted record
  int32_t use;         // the kept record: 0 the hypothesis's, 1 the refitted one
  int32_t total[2];    // the inliers of rec[0] and rec[1]
  int32_t pad;
  float rec[2][8];
};

// the call's constants of the inlier test
struct ShapeTest {
  int32_t kind, normal_test;
  float max_dist, c2;
};

enum { kShInit = 0, kShHyp = 1, kShRefit = 2 };        // what a tile count / scan is for
enum { kShToFirst = 0, kShToCand = 1, kShToNext = 2 };  // ... and a scatter

__global__ __launch_bounds__(256) void shapes_gather_kernel(const float4 *__restrict__ nodes, const uint32_t *__restrict__ inv,
                                                            int32_t n, const uint8_t *__restrict__ deleted,
                                                            const float *__restrict__ normals, float4 *__restrict__ P,
                                                            float4 *__restrict__ N, uint8_t *__restrict__ left,
                                                            int32_t *__restrict__ labels, int32_t *__restrict__ ids) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float nan = __builtin_nanf("");
  const float4 nd = node_at(nodes, inv[i]);
  const float4 m = float4{normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], 0.0f};
  const bool live = !(deleted && deleted[i]) && plane_point_live(nd.x, nd.y, nd.z) && plane_normal_live(m.x, m.y, m.z);
  P[i] = live ? float4{nd.x, nd.y, nd.z, 0.0f} : float4{nan, nan, nan, 0.0f};
  N[i] = live ? m : float4{nan, nan, nan, 0.0f};
  left[i] = live ? (uint8_t)1 : (uint8_t)0;
  labels[i] = -1;
  ids[i] = -1;
}

// n_hyp == 0 or Len() == 0: nothing runs, every row of every output is written
__global__ __launch_bounds__(256) void shapes_empty_kernel(int32_t n, int64_t rows, int32_t max_shapes,
                                                           int32_t *__restrict__ d_n_shapes, float *__restrict__ shapes,
                                                           int32_t *__restrict__ sizes, int32_t *__restrict__ refined,
                                                           int32_t *__restrict__ best, int32_t *__restrict__ labels,
                                                           int32_t *__restrict__ ids, int32_t *__restrict__ status,
                                                           int32_t *__restrict__ counts, float *__restrict__ hyp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *d_n_shapes = 0;
  if (i < n) {
    labels[i] = -1;
    if (ids) ids[i] = -1;
  }
  if (i < max_shapes) {
#pragma unroll
    for (int k = 0; k < 8; k++) shapes[8 * i + k] = 0.0f;
    sizes[i] = 0;
    refined[i] = 0;
    best[i] = -1;
  }
  if (i < rows) {
    if (status) status[i] = kShapeNotRun;
    if (counts) counts[i] = 0;
    if (hyp) {
#pragma unroll
      for (int k = 0; k < 8; k++) hyp[8 * i + k] = 0.0f;
    }
  }
}

// partner[h] = the id of hypothesis h's partner among the seed's radius neighbourhood, -1 where it has none
template <int kSrc>
__global__ __launch_bounds__(kShBlock) void shapes_partner_kernel(GridView g, TreeView tv, XTreeView xv, int64_t guard,
                                                                  const ShapeState *__restrict__ S,
                                                                  const int32_t *__restrict__ A, const float4 *__restrict__ P,
                                                                  const uint32_t *__restrict__ samples, int64_t n_hyp,
                                                                  float bound, const uint8_t *__restrict__ left,
                                                                  int32_t *__restrict__ partner) {
  extern __shared__ uint32_t s_stack[];
  if (!S->run) return;  // (uniform over the grid: the whole wave leaves)
  const int64_t h = (int64_t)blockIdx.x * kShBlock + threadIdx.x;
  const bool live = h < n_hyp;
  const int lane = (int)(threadIdx.x & 63u);
  uint32_t u1 = 0u, seed = 0xffffffffu;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (live) {
    const uint32_t i0 = pose_sample_index(samples[2 * h], (uint32_t)S->R);
    const float4 p = P[i0];
    seed = (uint32_t)A[i0];
    u1 = samples[2 * h + 1];
    qx = p.x; qy = p.y; qz = p.z;
  }
  const uint64_t none = ~0ull;
  uint64_t key = none;
  // the record p inside the bound of the seed sd with the word u: a candidate where it is left and not the seed.  The
  // key first, the flag only where the key would be a new minimum: of N records in any order about ln N are, so the
  // scattered byte load behind every record's own load (what the kernel waited for) is paid a dozen times, not N.
  auto consider = [&](uint64_t &k, const float4 &p, const uint32_t u, const uint32_t sd) {
    const uint32_t id = __float_as_uint(p.w);
    const uint64_t c = shape_partner_key(u, id);
    if (c < k && id != sd && left[id]) k = c;
  };
  radius_visit<kSrc>(
      RadiusViews{g, tv, xv, guard}, s_stack + threadIdx.x, kShBlock, qx, qy, qz, bound, live,
      [&](const float4 &p, float) { consider(key, p, u1, seed); },
      [&](int owner, float, float, float, auto rows) {  // this lane's share of the owner's fat row, then the wave's minimum
        const uint32_t ou = __shfl(u1, owner), os = __shfl(seed, owner);
        uint64_t part = none;
        rows([&](const float4 &p, float) { consider(part, p, ou, os); });
#pragma unroll
        for (int x = 1; x < 64; x <<= 1) {
          const uint64_t o = __shfl_xor(part, x);
          part = o < part ? o : part;
        }
        if (lane == owner) key = part < key ? part : key;
      });
  if (!live) return;
  partner[h] = key == none ? -1 : (int32_t)(uint32_t)key;
}

__global__ __launch_bounds__(256) void shapes_fit_kernel(const ShapeState *__restrict__ S, const int32_t *__restrict__ A,
                                                         const float4 *__restrict__ Pid, const float4 *__restrict__ Nid,
                                                         const uint32_t *__restrict__ samples,
                                                         const int32_t *__restrict__ partner, int64_t n_hyp, int32_t kind,
                                                         PlaneAxis ax, float r_min, float r_max,
                                                         int32_t *__restrict__ status, int32_t *__restrict__ counts,
                                                         float *__restrict__ hyp) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n_hyp) return;
  float rec[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  int32_t st = kShapeNotRun;
  if (S->run) {
    const uint32_t R = (uint32_t)S->R;
    const int32_t i0 = A[pose_sample_index(samples[2 * h], R)];
    // partner == nullptr: sample_radius == 0, the second word names the partner among all that is left
    const int32_t i1 = partner ? partner[h] : A[pose_sample_index(samples[2 * h + 1], R)];
    const bool has = i1 >= 0 && i1 != i0;
    const float4 p0 = Pid[i0], n0 = Nid[i0], p1 = Pid[has ? i1 : i0], n1 = Nid[has ? i1 : i0];
    st = shape_hypothesis(kind, has, &p0.x, &n0.x, &p1.x, &n1.x, ax, r_min, r_max, rec);
  }
  status[h] = st;
  counts[h] = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) hyp[8 * h + k] = rec[k];  // (the caller's array: no alignment beyond a float's)
}

template <int kKind, bool kNormalTest>
__global__ __launch_bounds__(kShBlock) void shapes_count_kernel(const ShapeState *__restrict__ S, const float4 *__restrict__ P,
                                                                const float4 *__restrict__ N, int64_t n_hyp,
                                                                const int32_t *__restrict__ status,
                                                                const float *__restrict__ hyp, float max_dist, float c2,
                                                                int32_t chunk, int32_t *__restrict__ counts) {
  if (!S->run) return;  // (uniform)
  const int64_t h0 = (int64_t)blockIdx.x * kShTile + threadIdx.x, h1 = h0 + kShBlock;
  const bool ok0 = h0 < n_hyp && status[h0] == kShapeOk, ok1 = h1 < n_hyp && status[h1] == kShapeOk;
  if (__ballot(ok0 || ok1) == 0ull) return;  // (wave-uniform)
  const int64_t len = S->R;
  const int64_t k0 = (int64_t)blockIdx.y * chunk;
  if (k0 >= len) return;
  const int64_t k1 = k0 + chunk < len ? k0 + chunk : len;
  const float *a = hyp + 8 * (h0 < n_hyp ? h0 : n_hyp - 1), *b = hyp + 8 * (h1 < n_hyp ? h1 : n_hyp - 1);
  const shape_f2 cx = {a[0], b[0]}, cy = {a[1], b[1]}, cz = {a[2], b[2]};
  const shape_f2 ax = {a[4], b[4]}, ay = {a[5], b[5]}, az = {a[6], b[6]};
  shape_f2 lo2, hi2;
  {
    float l, u;
    shape_band(a[3], max_dist, &l, &u);
    lo2.x = l; hi2.x = u;
    shape_band(b[3], max_dist, &l, &u);
    lo2.y = l; hi2.y = u;
  }
  const shape_f2 cc = {c2, c2};
  int32_t c0 = 0, c1 = 0;
#pragma unroll 4  // (four records' scalar loads in flight ahead of their arithmetic)
  for (int64_t k = k0; k < k1; k++) {
    const float4 p = P[k];  // (wave-uniform: a scalar load)
    const shape_f2 vx = shape_f2{p.x, p.x} - cx, vy = shape_f2{p.y, p.y} - cy, vz = shape_f2{p.z, p.z} - cz;
    shape_f2 d2 = (vx * vx + vy * vy) + vz * vz;
    shape_f2 t = {0.0f, 0.0f};
    if (kKind == kShapeCylinder) {
      t = (vx * ax + vy * ay) + vz * az;
      d2 = d2 - t * t;
    }
    bool in0 = d2.x < hi2.x && d2.x > lo2.x, in1 = d2.y < hi2.y && d2.y > lo2.y;
    if (kNormalTest) {
      const float4 m = N[k];
      const shape_f2 mx = {m.x, m.x}, my = {m.y, m.y}, mz = {m.z, m.z};
      shape_f2 gg = (mx * vx + my * vy) + mz * vz;
      if (kKind == kShapeCylinder) gg = gg - t * ((mx * ax + my * ay) + mz * az);
      const shape_f2 lhs = gg * gg, rhs = cc * d2;
      in0 = in0 && lhs.x >= rhs.x;
      in1 = in1 && lhs.y >= rhs.y;
    }
    c0 += in0 ? 1 : 0;
    c1 += in1 ? 1 : 0;
  }
  if (ok0 && c0) atomicAdd(&counts[h0], c0);
  if (ok1 && c1) atomicAdd(&counts[h1], c1);
}

__global__ __launch_bounds__(kShOneBlock) void shapes_select_kernel(ShapeState *__restrict__ S, int64_t n_hyp,
                                                                    const int32_t *__restrict__ status,
                                                                    const int32_t *__restrict__ counts,
                                                                    const float *__restrict__ hyp, int64_t min_inliers) {
  __shared__ uint64_t s_key[kShOneWaves];
  const int t = (int)threadIdx.x;
  const bool run = S->run != 0;
  // the first best: the largest count, the smallest h among equals; 0: no hypothesis has status 0
  uint64_t key = 0;
  if (run)
    for (int64_t h = t; h < n_hyp; h += kShOneBlock)
      if (status[h] == kShapeOk) {
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
  for (int w = 0; w < kShOneWaves; w++) key = s_key[w] > key ? s_key[w] : key;
  const int32_t best = key ? (int32_t)(~(uint32_t)key) : -1;
  const int32_t best_count = key ? (int32_t)((uint32_t)(key >> 32) - 1u) : 0;
  const int64_t need = min_inliers > 2 ? min_inliers : 2;
  const bool found = run && key && (int64_t)best_count >= need;
  S->found = found ? 1 : 0;
  S->best = best;
  S->best_count = best_count;
  S->cand_size = 0;
  S->refit_ok = 0;
  S->use = 0;
  S->total[0] = S->total[1] = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    S->rec[0][k] = found ? hyp[8 * (int64_t)best + k] : 0.0f;
    S->rec[1][k] = 0.0f;
  }
}

// ---- the ordered compaction

// a record and its band, as the kernels of the compaction hold it
struct ShapeRec {
  float v[8], lo2, hi2;
};
__device__ __forceinline__ ShapeRec shape_rec_load(const float *rec, const float max_dist) {
  ShapeRec r;
#pragma unroll
  for (int k = 0; k < 8; k++) r.v[k] = rec[k];
  shape_band(r.v[3], max_dist, &r.lo2, &r.hi2);
  return r;
}

// does entry i leave the list?  init: it is not live (its record is NaN); else: it is an inlier of rec
template <bool kIsInit>
__device__ __forceinline__ bool shapes_leaves(const float4 *__restrict__ P, const float4 *__restrict__ N, int64_t i,
                                              const ShapeRec &rec, const ShapeTest &T) {
  const float4 p = P[i];
  if (kIsInit) return !(p.x == p.x);
  const float4 m = N[i];
  return shape_inlier_any(T.kind, T.normal_test != 0, rec.v, rec.lo2, rec.hi2, T.c2, p.x, p.y, p.z, m.x, m.y, m.z);
}

template <int kMode>
__global__ __launch_bounds__(kScBlock) void shapes_tile_count_kernel(const ShapeState *__restrict__ S, int32_t n,
                                                                     const float4 *__restrict__ P,
                                                                     const float4 *__restrict__ N, ShapeTest T,
                                                                     int32_t *__restrict__ tile_cnt) {
  __shared__ int32_t s_w[kScBlock / 64];
  int64_t len = n;
  ShapeRec rec = {};
  if (kMode != kShInit) {
    if (!S->found || (kMode == kShRefit && !S->refit_ok)) return;  // (uniform)
    len = S->R;
    rec = shape_rec_load(S->rec[kMode == kShRefit ? 1 : 0], T.max_dist);
  }
  const int64_t base = (int64_t)blockIdx.x * kScTile;
  if (base >= len) return;  // (uniform; the scan reads the tiles below len only)
  int32_t c = 0;
#pragma unroll
  for (int j = 0; j < kScIters; j++) {
    const int64_t i = base + j * kScBlock + threadIdx.x;
    if (i < len) c += shapes_leaves<kMode == kShInit>(P, N, i, rec, T) ? 1 : 0;
  }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) c += __shfl_xor(c, x);
  if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kScBlock / 64; w++) sum += s_w[w];
    tile_cnt[blockIdx.x] = sum;
  }
}

// ONE workgroup: tile_off = the exclusive scan of tile_cnt over the tiles of the list, and what the total decides
template <int kMode>
__global__ __launch_bounds__(kShOneBlock) void shapes_scan_kernel(ShapeState *__restrict__ S, int32_t n, int32_t refine,
                                                                  const int32_t *__restrict__ tile_cnt,
                                                                  int32_t *__restrict__ tile_off) {
  __shared__ uint32_t s_w[kShOneWaves];
  const int t = (int)threadIdx.x, wave = t >> 6;
  int64_t len = n;
  if (kMode != kShInit) {
    if (!S->found || (kMode == kShRefit && !S->refit_ok)) return;  // (uniform)
    len = S->R;
  }
  const int32_t tiles = (int32_t)((len + kScTile - 1) / kScTile);
  uint32_t carry = 0u;
  for (int32_t b = 0; b < tiles; b += kShOneBlock) {  // uniform
    const int32_t i = b + t;
    const uint32_t v = i < tiles ? (uint32_t)tile_cnt[i] : 0u;
    const uint32_t incl = wave_incl_scan_u32(v);
    if ((t & 63) == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < kShOneWaves; w++) {
      const uint32_t c = s_w[w];
      before += w < wave ? c : 0u;
      total += c;
    }
    __syncthreads();
    if (i < tiles) tile_off[i] = (int32_t)(carry + before + incl - v);
    carry += total;
  }
  if (t != 0) return;
  if (kMode == kShInit) {
    const int32_t R = n - (int32_t)carry;
    S->R = R;
    S->run = R >= 2 ? 1 : 0;
  } else if (kMode == kShHyp) {
    S->total[0] = (int32_t)carry;
    if (refine) S->cand_size = (int32_t)carry;
  } else {
    S->total[1] = (int32_t)carry;
    S->use = (int32_t)carry >= S->best_count ? 1 : 0;
  }
}

// kShToFirst: the live ids of [0, n) and their records -> A_0.  kShToCand: the inliers of the hypothesis's record -> the
// candidate list.  kShToNext: the inliers of the kept record -> ids behind the earlier rounds', their labels, their left
// flag cleared; the rest -> A_{r+1}.  A == nullptr: entry i is id i.
template <int kMode>
__global__ __launch_bounds__(kScBlock) void shapes_scatter_kernel(const ShapeState *__restrict__ S, int32_t n, int32_t round,
                                                                  const int32_t *__restrict__ A, const float4 *__restrict__ P,
                                                                  const float4 *__restrict__ N, ShapeTest T,
                                                                  const int32_t *__restrict__ tile_off0,
                                                                  const int32_t *__restrict__ tile_off1,
                                                                  int32_t *__restrict__ A_out, float4 *__restrict__ P_out,
                                                                  float4 *__restrict__ N_out, int32_t *__restrict__ list,
                                                                  int32_t *__restrict__ labels, uint8_t *__restrict__ left) {
  __shared__ uint32_t s_w[kScBlock / 64];
  const int t = (int)threadIdx.x, wave = t >> 6;
  int64_t len = n;
  ShapeRec rec = {};
  const int32_t *tile_off = tile_off0;
  int32_t list_at = 0;
  if (kMode != kShToFirst) {
    if (!S->found) return;  // (uniform)
    len = S->R;
    const int use = kMode == kShToNext ? S->use : 0;
    tile_off = use ? tile_off1 : tile_off0;
    rec = shape_rec_load(S->rec[use], T.max_dist);
    if (kMode == kShToNext) list_at = S->off;
  }
  const int64_t base = (int64_t)blockIdx.x * kScTile;
  if (base >= len) return;  // (uniform)
  uint32_t gone = (uint32_t)tile_off[blockIdx.x];  // entries that left before this stretch
#pragma unroll 1
  for (int j = 0; j < kScIters; j++) {
    const int64_t i = base + j * kScBlock + t;
    const bool valid = i < len;
    const bool leaves = valid && shapes_leaves<kMode == kShToFirst>(P, N, i, rec, T);
    const uint32_t incl = wave_incl_scan_u32(leaves ? 1u : 0u);
    if ((t & 63) == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < kScBlock / 64; w++) {
      const uint32_t c = s_w[w];
      before += w < wave ? c : 0u;
      total += c;
    }
    __syncthreads();
    const uint32_t pos = gone + before + incl - (leaves ? 1u : 0u);  // entries before i that leave
    if (valid) {
      const int32_t id = A ? A[i] : (int32_t)i;
      if (leaves) {
        if (kMode != kShToFirst) list[(int64_t)list_at + pos] = id;
        if (kMode == kShToNext) {
          labels[id] = round;
          left[id] = (uint8_t)0;
        }
      } else if (kMode != kShToCand) {
        const int64_t o = i - (int64_t)pos;
        A_out[o] = id;
        P_out[o] = P[i];
        N_out[o] = N[i];
      }
    }
    gone += total;
  }
}

// ---- the refit

// partial[13 tile ..]: the sums' terms over the tile's entries of the candidate list, added in a fixed order
__global__ __launch_bounds__(kScBlock) void shapes_sums_kernel(const ShapeState *__restrict__ S, int32_t kind,
                                                               const int32_t *__restrict__ cand,
                                                               const float4 *__restrict__ Pid,
                                                               double *__restrict__ partial) {
  __shared__ double s_w[kScBlock / 64][kShapeSums];
  if (!S->found) return;  // (uniform)
  const int64_t len = S->cand_size;
  const int64_t base = (int64_t)blockIdx.x * kScTile;
  if (base >= len) return;  // (uniform)
  float rec[8];
#pragma unroll
  for (int k = 0; k < 8; k++) rec[k] = S->rec[0][k];
  double s[kShapeSums];
#pragma unroll
  for (int k = 0; k < kShapeSums; k++) s[k] = 0.0;
#pragma unroll 1
  for (int j = 0; j < kScIters; j++) {
    const int64_t i = base + j * kScBlock + threadIdx.x;
    if (i < len) {
      const float4 p = Pid[cand[i]];
      double x[3], term[kShapeSums];
      shape_refit_coords(kind, rec, &p.x, x);
      shape_refit_terms(x, term);
#pragma unroll
      for (int k = 0; k < kShapeSums; k++) s[k] += term[k];
    }
  }
#pragma unroll
  for (int k = 0; k < kShapeSums; k++) {
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) s[k] += __shfl_xor(s[k], x);
  }
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (int k = 0; k < kShapeSums; k++) s_w[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < kShapeSums) {
    double sum = s_w[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kScBlock / 64; w++) sum += s_w[w][threadIdx.x];
    partial[(int64_t)blockIdx.x * kShapeSums + threadIdx.x] = sum;
  }
}

// one wave: lane k < 13 adds sum k's tile partials in tile order; lane 0 solves
__global__ __launch_bounds__(64) void shapes_refit_kernel(ShapeState *__restrict__ S, int32_t kind,
                                                          const double *__restrict__ partial, float r_min, float r_max) {
  __shared__ double s_sum[kShapeSums];
  if (!S->found) return;  // (uniform)
  const int64_t len = S->cand_size;
  const int64_t tiles = (len + kScTile - 1) / kScTile;
  if (threadIdx.x < kShapeSums) {
    double sum = 0.0;
    for (int64_t b = 0; b < tiles; b++) sum += partial[b * kShapeSums + threadIdx.x];
    s_sum[threadIdx.x] = sum;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float rec[8], out[8];
  double s[kShapeSums];
#pragma unroll
  for (int k = 0; k < 8; k++) rec[k] = S->rec[0][k];
#pragma unroll
  for (int k = 0; k < kShapeSums; k++) s[k] = s_sum[k];
  const bool ok = len > 0 && shape_refit(kind, rec, (double)len, s, r_min, r_max, out);
  S->refit_ok = ok ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 8; k++) S->rec[1][k] = ok ? out[k] : 0.0f;
}

__global__ __launch_bounds__(64) void shapes_round_end_kernel(ShapeState *__restrict__ S, int32_t round,
                                                              int32_t *__restrict__ d_n_shapes, float *__restrict__ shapes,
                                                              int32_t *__restrict__ sizes, int32_t *__restrict__ refined,
                                                              int32_t *__restrict__ best) {
  if (threadIdx.x != 0) return;
  const bool found = S->found != 0;
  const int use = found ? S->use : 0;
  const int32_t size = found ? S->total[use] : 0;
#pragma unroll
  for (int k = 0; k < 8; k++) shapes[8 * (int64_t)round + k] = found ? S->rec[use][k] : 0.0f;
  sizes[round] = size;
  refined[round] = use;
  best[round] = found ? S->best : -1;
  if (found) *d_n_shapes = round + 1;
  const int32_t R = S->R - size;
  S->off += size;
  S->R = R;
  S->run = found && R >= 2 ? 1 : 0;
  S->found = 0;
}

template <int kSrc>
void partner_launch(const pcgx_kdtree *t, const TreeView &tv, const XTreeView &xv, size_t stack_bytes, const ShapeState *S,
                    const int32_t *A, const float4 *P, const uint32_t *samples, int64_t n_hyp, float bound,
                    const uint8_t *left, int32_t *partner, hipStream_t st) {
  const dim3 grid((unsigned)((n_hyp + kShBlock - 1) / kShBlock)), block(kShBlock);
  const GridView g = kSrc == kRangeGrid ? t->grid : GridView{};
  hipLaunchKernelGGL(shapes_partner_kernel<kSrc>, grid, block, stack_bytes, st, g, tv, xv, xwalk_guard(t->n), S, A, P, samples,
                     n_hyp, bound, left, partner);
}

template <int kKind, bool kNormalTest>
void count_launch(dim3 grid, const ShapeState *S, const float4 *P, const float4 *N, int64_t n_hyp, const int32_t *status,
                  const float *hyp, float max_dist, float c2, int32_t chunk, int32_t *counts, hipStream_t st) {
  hipLaunchKernelGGL((shapes_count_kernel<kKind, kNormalTest>), grid, dim3(kShBlock), 0, st, S, P, N, n_hyp, status, hyp,
                     max_dist, c2, chunk, counts);
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kShapesMaxRows = 0x7fffffff;
constexpr int32_t kShapesMaxShapes = 256;

pcgx_status shapes_check(const char *fn, const pcgx_kdtree *t, int32_t kind, const void *samples, int64_t n_hyp,
                         int32_t max_shapes, float max_dist, int64_t min_inliers, float sample_radius, float r_min,
                         float r_max, const float *axis, float min_axis_cos, const void *normals, float min_normal_cos) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (kind != kShapeSphere && kind != kShapeCylinder)
    return fail(PCGX_E_INVALID, "%s: kind must be PCGX_SHAPE_SPHERE or PCGX_SHAPE_CYLINDER", fn);
  if (n_hyp < 0) return fail(PCGX_E_INVALID, "%s: negative number of hypotheses", fn);
  if (max_shapes < 1 || max_shapes > kShapesMaxShapes)
    return fail(PCGX_E_INVALID, "%s: max_shapes must be in [1, %d]", fn, kShapesMaxShapes);
  if (!(max_dist > 0.0f) || !(max_dist < __builtin_inff()))
    return fail(PCGX_E_INVALID, "%s: max_dist must be finite and > 0", fn);
  if (min_inliers < 0) return fail(PCGX_E_INVALID, "%s: negative min_inliers", fn);
  if (!(sample_radius >= 0.0f) || !(sample_radius < __builtin_inff()))
    return fail(PCGX_E_INVALID, "%s: sample_radius must be finite and >= 0", fn);
  if (!(r_min >= 0.0f) || !(r_max >= 0.0f) || !(r_min <= r_max))
    return fail(PCGX_E_INVALID, "%s: 0 <= r_min <= r_max is required", fn);
  if (axis) {
    if (!plane_point_live(axis[0], axis[1], axis[2]) || (axis[0] == 0.0f && axis[1] == 0.0f && axis[2] == 0.0f))
      return fail(PCGX_E_INVALID, "%s: the axis must be finite and not zero", fn);
    if (!(min_axis_cos >= 0.0f) || !(min_axis_cos <= 1.0f))
      return fail(PCGX_E_INVALID, "%s: min_axis_cos must be in [0, 1]", fn);
  }
  if (!(min_normal_cos >= 0.0f) || !(min_normal_cos <= 1.0f))
    return fail(PCGX_E_INVALID, "%s: min_normal_cos must be in [0, 1]", fn);
  if (t->n > 0 && !normals) return fail(PCGX_E_INVALID, "%s: NULL normals (the hypotheses are made from them)", fn);
  if (n_hyp > 0 && !samples) return fail(PCGX_E_INVALID, "%s: NULL samples", fn);
  if (n_hyp > kShapesMaxRows / max_shapes)
    return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 hypotheses over all rounds", fn);
  if (t->n > kShapesMaxRows) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points", fn);
  return PCGX_OK;
}

// PCGX_SHAPES_SPLIT=<n>: the number of chunks of the points, forced (tests of the merge, measurements).  Read per call.
int32_t shapes_split(int64_t n_hyp, int64_t n) {
  const char *e = getenv("PCGX_SHAPES_SPLIT");
  if (e && *e) {
    const long v = atol(e);
    if (v > 0) return (int32_t)(v < kShMaxSplit ? v : kShMaxSplit);
  }
  const int64_t tiles = (n_hyp + kShTile - 1) / kShTile;
  int64_t s = (kShTargetWaves + tiles - 1) / tiles;
  const int64_t cap = n / kShMinChunk;
  if (s > cap) s = cap;
  if (s > kShMaxSplit) s = kShMaxSplit;
  return (int32_t)(s < 1 ? 1 : s);
}

}  // namespace

extern "C" int32_t pcgx_shapes_tile(void) { return kShTile; }

extern "C" pcgx_status pcgx_kdtree_shapes_dev(const pcgx_kdtree *t, int32_t kind, const uint32_t *d_samples, int64_t n_hyp,
                                              int32_t max_shapes, float max_dist, int64_t min_inliers, float sample_radius,
                                              float r_min, float r_max, const float *axis, float min_axis_cos,
                                              const float *d_normals, float min_normal_cos, int32_t refine,
                                              int32_t *d_n_shapes, float *d_shapes, int32_t *d_sizes, int32_t *d_refined,
                                              int32_t *d_best, int32_t *d_labels, int32_t *d_ids, int32_t *d_status,
                                              int32_t *d_counts, float *d_hyp_shapes, void *stream) {
  PCGX_API_LOCK();
  const char *fn = "pcgx_kdtree_shapes_dev";
  PCGX_TRY(shapes_check(fn, t, kind, d_samples, n_hyp, max_shapes, max_dist, min_inliers, sample_radius, r_min, r_max, axis,
                        min_axis_cos, d_normals, min_normal_cos));
  const int64_t n = t->n;
  if (!d_n_shapes || !d_shapes || !d_sizes || !d_refined || !d_best || (n > 0 && !d_labels))
    return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  const int64_t rows = n_hyp * max_shapes;
  if (n == 0 || n_hyp == 0) {
    int64_t most = n > rows ? n : rows;
    if (most < max_shapes) most = max_shapes;
    hipLaunchKernelGGL(shapes_empty_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, st, (int32_t)n, rows,
                       max_shapes, d_n_shapes, d_shapes, d_sizes, d_refined, d_best, d_labels, d_ids, d_status, d_counts,
                       d_hyp_shapes);
    PCGX_HIP_TRY(hipGetLastError());
    return PCGX_OK;
  }
  Arena &ar = ctx().arena;
  PCGX_TRY(ar.begin(st));
  const uint32_t *inv = nullptr;
  PCGX_TRY(range_inverse_map(t, &inv, st));
  const bool local = sample_radius > 0.0f;
  const RangeSrc src = range_source(t);  // as pcgx_kdtree_range_count takes it
  XTreeView xv{};
  if (local && src == kRangeXWalk) PCGX_TRY(xtree_view(t, &xv, st));
  const TreeView tv = t->view();
  const int32_t ni = (int32_t)n;
  const size_t N = (size_t)n;
  const unsigned tiles = (unsigned)((n + kScTile - 1) / kScTile);
  // the lists and records of two rounds in turn (round r reads [r & 1], writes the other), and the records by id
  int32_t *A[2] = {nullptr, nullptr}, *cand = nullptr, *tile_cnt = nullptr, *tile_off[2] = {nullptr, nullptr},
          *partner = nullptr;
  float4 *P[2] = {nullptr, nullptr}, *Nr[2] = {nullptr, nullptr}, *Pid = nullptr, *Nid = nullptr;
  ShapeState *S = nullptr;
  double *partial = nullptr;
  uint8_t *d_deleted = nullptr, *left = nullptr;
  for (int k = 0; k < 2; k++) {
    PCGX_TRY(ar.alloc_n(N, &A[k]));
    PCGX_TRY(ar.alloc_n(N, &P[k]));
    PCGX_TRY(ar.alloc_n(N, &Nr[k]));
    PCGX_TRY(ar.alloc_n((size_t)tiles, &tile_off[k]));
  }
  PCGX_TRY(ar.alloc_n(N, &Pid));
  PCGX_TRY(ar.alloc_n(N, &Nid));
  PCGX_TRY(ar.alloc_n(N, &left));
  PCGX_TRY(ar.alloc_n((size_t)tiles, &tile_cnt));
  if (refine) {
    PCGX_TRY(ar.alloc_n(N, &cand));
    PCGX_TRY(ar.alloc_n((size_t)tiles * kShapeSums, &partial));
  }
  if (local) PCGX_TRY(ar.alloc_n((size_t)n_hyp, &partner));
  PCGX_TRY(ar.alloc_n(1, &S));
  if (!d_ids) PCGX_TRY(ar.alloc_n(N, &d_ids));
  // an optional per-hypothesis output that is not wanted: one round's rows, used by every round in turn
  const int64_t st_stride = d_status ? n_hyp : 0, cn_stride = d_counts ? n_hyp : 0, hp_stride = d_hyp_shapes ? n_hyp : 0;
  if (!d_status) PCGX_TRY(ar.alloc_n((size_t)n_hyp, &d_status));
  if (!d_counts) PCGX_TRY(ar.alloc_n((size_t)n_hyp, &d_counts));
  if (!d_hyp_shapes) PCGX_TRY(ar.alloc_n((size_t)n_hyp * 8, &d_hyp_shapes));
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
  const bool normal_test = min_normal_cos != 0.0f;
  const ShapeTest T{kind, normal_test ? 1 : 0, max_dist, min_normal_cos * min_normal_cos};
  const float bound = sample_radius * sample_radius;
  size_t stack_bytes = 0;
  if (local && src == kRangeXWalk) stack_bytes = xwalk_stack_bytes(xv, kShBlock);
  else if (local && src == kRangeWalk) stack_bytes = walk_stack_bytes(tv, kShBlock);
  PCGX_HIP_TRY(hipMemsetAsync(S, 0, sizeof(ShapeState), st));
  PCGX_HIP_TRY(hipMemsetAsync(d_n_shapes, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(shapes_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t->d_nodes, inv, ni,
                     (const uint8_t *)d_deleted, d_normals, Pid, Nid, left, d_labels, d_ids);
  hipLaunchKernelGGL(shapes_tile_count_kernel<kShInit>, dim3(tiles), dim3(kScBlock), 0, st, (const ShapeState *)S, ni,
                     (const float4 *)Pid, (const float4 *)Nid, T, tile_cnt);
  hipLaunchKernelGGL(shapes_scan_kernel<kShInit>, dim3(1), dim3(kShOneBlock), 0, st, S, ni, refine,
                     (const int32_t *)tile_cnt, tile_off[0]);
  hipLaunchKernelGGL(shapes_scatter_kernel<kShToFirst>, dim3(tiles), dim3(kScBlock), 0, st, (const ShapeState *)S, ni, 0,
                     (const int32_t *)nullptr, (const float4 *)Pid, (const float4 *)Nid, T, (const int32_t *)tile_off[0],
                     (const int32_t *)tile_off[1], A[0], P[0], Nr[0], (int32_t *)nullptr, (int32_t *)nullptr,
                     (uint8_t *)nullptr);
  const int32_t split = shapes_split(n_hyp, n);
  int64_t chunk = (n + split - 1) / split;
  if (chunk < 1) chunk = 1;
  const dim3 count_grid((unsigned)((n_hyp + kShTile - 1) / kShTile), (unsigned)((n + chunk - 1) / chunk));
  const unsigned fit_blocks = (unsigned)((n_hyp + 255) / 256);
  for (int32_t r = 0; r < max_shapes; r++) {
    const int in = r & 1, out = in ^ 1;
    int32_t *status = d_status + st_stride * r, *counts = d_counts + cn_stride * r;
    float *hyp = d_hyp_shapes + 8 * hp_stride * r;
    const float4 *Pi = P[in], *Ni = Nr[in];
    const int32_t *Ai = A[in];
    const uint32_t *smp = d_samples + 2 * n_hyp * r;
    if (local) {
      if (src == kRangeXWalk)
        partner_launch<kRangeXWalk>(t, tv, xv, stack_bytes, S, Ai, Pi, smp, n_hyp, bound, left, partner, st);
      else if (src == kRangeGrid)
        partner_launch<kRangeGrid>(t, tv, xv, stack_bytes, S, Ai, Pi, smp, n_hyp, bound, left, partner, st);
      else
        partner_launch<kRangeWalk>(t, tv, xv, stack_bytes, S, Ai, Pi, smp, n_hyp, bound, left, partner, st);
    }
    hipLaunchKernelGGL(shapes_fit_kernel, dim3(fit_blocks), dim3(256), 0, st, (const ShapeState *)S, Ai, (const float4 *)Pid,
                       (const float4 *)Nid, smp, (const int32_t *)partner, n_hyp, kind, ax, r_min, r_max, status, counts, hyp);
    if (kind == kShapeSphere) {
      if (normal_test)
        count_launch<kShapeSphere, true>(count_grid, S, Pi, Ni, n_hyp, status, hyp, max_dist, T.c2, (int32_t)chunk, counts, st);
      else
        count_launch<kShapeSphere, false>(count_grid, S, Pi, Ni, n_hyp, status, hyp, max_dist, T.c2, (int32_t)chunk, counts, st);
    } else {
      if (normal_test)
        count_launch<kShapeCylinder, true>(count_grid, S, Pi, Ni, n_hyp, status, hyp, max_dist, T.c2, (int32_t)chunk, counts, st);
      else
        count_launch<kShapeCylinder, false>(count_grid, S, Pi, Ni, n_hyp, status, hyp, max_dist, T.c2, (int32_t)chunk, counts, st);
    }
    hipLaunchKernelGGL(shapes_select_kernel, dim3(1), dim3(kShOneBlock), 0, st, S, n_hyp, (const int32_t *)status,
                       (const int32_t *)counts, (const float *)hyp, min_inliers);
    hipLaunchKernelGGL(shapes_tile_count_kernel<kShHyp>, dim3(tiles), dim3(kScBlock), 0, st, (const ShapeState *)S, ni, Pi, Ni,
                       T, tile_cnt);
    hipLaunchKernelGGL(shapes_scan_kernel<kShHyp>, dim3(1), dim3(kShOneBlock), 0, st, S, ni, refine,
                       (const int32_t *)tile_cnt, tile_off[0]);
    if (refine) {
      hipLaunchKernelGGL(shapes_scatter_kernel<kShToCand>, dim3(tiles), dim3(kScBlock), 0, st, (const ShapeState *)S, ni, r, Ai,
                         Pi, Ni, T, (const int32_t *)tile_off[0], (const int32_t *)tile_off[1], (int32_t *)nullptr,
                         (float4 *)nullptr, (float4 *)nullptr, cand, (int32_t *)nullptr, (uint8_t *)nullptr);
      hipLaunchKernelGGL(shapes_sums_kernel, dim3(tiles), dim3(kScBlock), 0, st, (const ShapeState *)S, kind,
                         (const int32_t *)cand, (const float4 *)Pid, partial);
      hipLaunchKernelGGL(shapes_refit_kernel, dim3(1), dim3(64), 0, st, S, kind, (const double *)partial, r_min, r_max);
      hipLaunchKernelGGL(shapes_tile_count_kernel<kShRefit>, dim3(tiles), dim3(kScBlock), 0, st, (const ShapeState *)S, ni, Pi,
                         Ni, T, tile_cnt);
      hipLaunchKernelGGL(shapes_scan_kernel<kShRefit>, dim3(1), dim3(kShOneBlock), 0, st, S, ni, refine,
                         (const int32_t *)tile_cnt, tile_off[1]);
    }
    hipLaunchKernelGGL(shapes_scatter_kernel<kShToNext>, dim3(tiles), dim3(kScBlock), 0, st, (const ShapeState *)S, ni, r, Ai,
                       Pi, Ni, T, (const int32_t *)tile_off[0], (const int32_t *)tile_off[1], A[out], P[out], Nr[out], d_ids,
                       d_labels, left);
    hipLaunchKernelGGL(shapes_round_end_kernel, dim3(1), dim3(64), 0, st, S, r, d_n_shapes, d_shapes, d_sizes, d_refined,
                       d_best);
  }
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_kdtree_shapes(const pcgx_kdtree *t, int32_t kind, const uint32_t *samples, int64_t n_hyp,
                                          int32_t max_shapes, float max_dist, int64_t min_inliers, float sample_radius,
                                          float r_min, float r_max, const float *axis, float min_axis_cos,
                                          const float *normals, float min_normal_cos, int32_t refine, int64_t *n_shapes,
                                          float *shapes, int64_t *sizes, int32_t *refined, int64_t *best, int64_t *labels,
                                          int64_t *ids, int32_t *status, int64_t *counts, float *hyp_shapes) {
  PCGX_API_CALL();
  const char *fn = "pcgx_kdtree_shapes";
  PCGX_TRY(shapes_check(fn, t, kind, samples, n_hyp, max_shapes, max_dist, min_inliers, sample_radius, r_min, r_max, axis,
                        min_axis_cos, normals, min_normal_cos));
  const int64_t n = t->n;
  if (!n_shapes || !shapes || !sizes || !refined || !best || (n > 0 && !labels))
    return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  const size_t N = (size_t)n, M = (size_t)max_shapes, H = (size_t)(n_hyp * max_shapes);
  // one block of int32 words: n_shapes, sizes, refined, best, labels, ids; then the per-hypothesis rows
  const size_t words = 1 + 3 * M + 2 * N;
  int32_t *d_out = nullptr, *d_status = nullptr, *d_counts = nullptr;
  float *d_shapes = nullptr, *d_hyp = nullptr, *d_normals = nullptr;
  uint32_t *d_samples = nullptr;
  PCGX_TRY(ha.alloc_n(words, &d_out));
  PCGX_TRY(ha.alloc_n(8 * M, &d_shapes));
  if (status && H) PCGX_TRY(ha.alloc_n(H, &d_status));
  if (counts && H) PCGX_TRY(ha.alloc_n(H, &d_counts));
  if (hyp_shapes && H) PCGX_TRY(ha.alloc_n(8 * H, &d_hyp));
  if (H) {
    PCGX_TRY(ha.alloc_n(2 * H, &d_samples));
    PCGX_TRY(staged_upload(d_samples, samples, 8 * H, st));
  }
  if (N) {
    PCGX_TRY(ha.alloc_n(3 * N, &d_normals));
    PCGX_TRY(staged_upload(d_normals, normals, 12 * N, st));
  }
  int32_t *d_sizes = d_out + 1, *d_refined = d_sizes + M, *d_best = d_refined + M, *d_labels = d_best + M,
          *d_ids = d_labels + N;
  PCGX_TRY(pcgx_kdtree_shapes_dev(t, kind, d_samples, n_hyp, max_shapes, max_dist, min_inliers, sample_radius, r_min, r_max,
                                  axis, min_axis_cos, d_normals, min_normal_cos, refine, d_out, d_shapes, d_sizes, d_refined,
                                  d_best, d_labels, d_ids, d_status, d_counts, d_hyp, st));
  RawVector<int32_t> r(words);
  PCGX_TRY(staged_download(r.data(), d_out, words * 4, st));
  PCGX_TRY(staged_download(shapes, d_shapes, 32 * M, st));
  *n_shapes = r[0];
  for (size_t k = 0; k < M; k++) {
    sizes[k] = r[1 + k];
    refined[k] = r[1 + M + k];
    best[k] = r[1 + 2 * M + k];
  }
  for (size_t i = 0; i < N; i++) labels[i] = r[1 + 3 * M + i];
  if (ids)
    for (size_t i = 0; i < N; i++) ids[i] = r[1 + 3 * M + N + i];
  if (status && H) PCGX_TRY(staged_download(status, d_status, H * 4, st));
  if (hyp_shapes && H) PCGX_TRY(staged_download(hyp_shapes, d_hyp, H * 32, st));
  if (counts && H) {
    RawVector<int32_t> c(H);
    PCGX_TRY(staged_download(c.data(), d_counts, H * 4, st));
    for (size_t i = 0; i < H; i++) counts[i] = c[i];
  }
  return PCGX_OK;
}
