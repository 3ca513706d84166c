// shapes.hip -- cylinder and sphere segmentation: the shape most of the cloud agrees on, by sample consensus over
// hypotheses made from two oriented points (Schnabel et al. 2007), the second drawn from the first's radius
// neighbourhood; its inliers taken out, then the next one (extension: no reference parity; include/pcgx.h, "shapes").
// The contract is planes.hip's: the caller draws every random word.  The rounds -- the device words they hand on, the
// select, the ordered compaction of the points that are left, the round end -- are consensus_peel.h's, over ShapeModel;
// the records by id stay for the whole call (32 bytes a point) beside a by-id "still left" flag, which the scatter to
// the next round clears for the inliers.  This file's own:
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
//   shapes_sums_kernel        the refit's sums over the candidate inlier list: a tile of 1024 a workgroup, a lane's four
//                             entries in order, a fixed shuffle tree, the four waves in order -> 13 doubles a tile.
//   shapes_refit_kernel       one wave adds the tile partials in tile order, one lane solves (shape_terms.h's shape_refit).
// Integer atomics only: the same input gives the same bits on every call, whatever the split.
#include <math.h>
#include <string.h>

#include "consensus_peel.h"
#include "radius_visit.h"
#include "shape_terms.h"

namespace pcgx {

constexpr int kShBlock = kRangeWalkBlock;  // one wave per workgroup (the walks' LDS frame stacks are [level][64])
constexpr int kShTile = kPeelTile;         // hypotheses per workgroup of the count
constexpr int kScBlock = kCpBlock, kScIters = kCpIters, kScTile = kCpTile;  // the sums go by the compaction's tiles
static_assert(kShBlock == kPeelBlock, "one wave per workgroup");
static_assert(kShapeNotRun == kPeelNotRun && kShapeOk == kPeelOk, "the status codes the rounds read");

typedef float shape_f2 __attribute__((ext_vector_type(2)));

// the call's constants of the inlier test
struct ShapeTest {
  int32_t kind, normal_test;
  float max_dist, c2;
};

// a record and its band, as the kernels of the compaction hold it
struct ShapeRec {
  float v[8], lo2, hi2;
};

struct ShapeModel {
  static constexpr int kRec = 8, kMinSample = 2;
  typedef ShapeTest Test;
  typedef ShapeRec Rec;
  static __device__ __forceinline__ Rec load(const float *rec, const Test &T) {
    ShapeRec r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.v[k] = rec[k];
    shape_band(r.v[3], T.max_dist, &r.lo2, &r.hi2);
    return r;
  }
  static __device__ __forceinline__ bool inlier(const Rec &rec, const Test &T, float4 p, const float4 *__restrict__ N,
                                                int64_t i) {
    const float4 m = N[i];
    return shape_inlier_any(T.kind, T.normal_test != 0, rec.v, rec.lo2, rec.hi2, T.c2, p.x, p.y, p.z, m.x, m.y, m.z);
  }
};
typedef PeelState<ShapeModel::kRec> ShapeState;

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

pcgx_status shapes_check(const char *fn, const pcgx_kdtree *t, int32_t kind, const void *samples, int64_t n_hyp,
                         int32_t max_shapes, float max_dist, int64_t min_inliers, float sample_radius, float r_min,
                         float r_max, const float *axis, float min_axis_cos, const void *normals, float min_normal_cos) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (kind != kShapeSphere && kind != kShapeCylinder)
    return fail(PCGX_E_INVALID, "%s: kind must be PCGX_SHAPE_SPHERE or PCGX_SHAPE_CYLINDER", fn);
  PCGX_TRY(peel_check_counts(fn, n_hyp, "max_shapes", max_shapes, max_dist, min_inliers));
  if (!(sample_radius >= 0.0f) || !(sample_radius < __builtin_inff()))
    return fail(PCGX_E_INVALID, "%s: sample_radius must be finite and >= 0", fn);
  if (!(r_min >= 0.0f) || !(r_max >= 0.0f) || !(r_min <= r_max))
    return fail(PCGX_E_INVALID, "%s: 0 <= r_min <= r_max is required", fn);
  PCGX_TRY(peel_check_axis(fn, axis, min_axis_cos));
  if (!(min_normal_cos >= 0.0f) || !(min_normal_cos <= 1.0f))
    return fail(PCGX_E_INVALID, "%s: min_normal_cos must be in [0, 1]", fn);
  if (t->n > 0 && !normals) return fail(PCGX_E_INVALID, "%s: NULL normals (the hypotheses are made from them)", fn);
  return peel_check_sizes(fn, t, samples, n_hyp, max_shapes);
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
  PeelOut o{d_n_shapes, d_shapes, d_sizes, d_refined, d_best, d_labels, d_ids, d_status, d_counts, d_hyp_shapes};
  if (n == 0 || n_hyp == 0) return peel_empty<ShapeModel::kRec>(n, n_hyp * max_shapes, max_shapes, o, st);
  Arena &ar = ctx().arena;
  PCGX_TRY(ar.begin(st));
  const uint32_t *inv = nullptr;
  PCGX_TRY(range_inverse_map(t, &inv, st));
  const bool local = sample_radius > 0.0f;
  const RangeSrc src = range_source(t);  // as pcgx_kdtree_range_count takes it
  XTreeView xv{};
  if (local && src == kRangeXWalk) PCGX_TRY(xtree_view(t, &xv, st));
  const TreeView tv = t->view();
  const size_t N = (size_t)n;
  PeelBuffers<ShapeModel::kRec> b;
  PCGX_TRY(peel_buffers(t, ar, n_hyp, true, refine != 0, &o, &b, st));
  // the records by id, the by-id "still left" flag, the refit's tile sums, the partners
  int32_t *partner = nullptr;
  float4 *Pid = nullptr, *Nid = nullptr;
  double *partial = nullptr;
  uint8_t *left = nullptr;
  PCGX_TRY(ar.alloc_n(N, &Pid));
  PCGX_TRY(ar.alloc_n(N, &Nid));
  PCGX_TRY(ar.alloc_n(N, &left));
  if (refine) PCGX_TRY(ar.alloc_n((size_t)b.tiles * kShapeSums, &partial));
  if (local) PCGX_TRY(ar.alloc_n((size_t)n_hyp, &partner));
  const PlaneAxis ax = plane_axis(axis, min_axis_cos);
  const bool normal_test = min_normal_cos != 0.0f;
  const ShapeTest T{kind, normal_test ? 1 : 0, max_dist, min_normal_cos * min_normal_cos};
  const float bound = sample_radius * sample_radius;
  size_t stack_bytes = 0;
  if (local && src == kRangeXWalk) stack_bytes = xwalk_stack_bytes(xv, kShBlock);
  else if (local && src == kRangeWalk) stack_bytes = walk_stack_bytes(tv, kShBlock);
  PCGX_TRY(peel_first<ShapeModel>(t, inv, b, T, d_normals, Pid, Nid, left, o, st));
  int32_t chunk = 0;
  const dim3 count_grid = peel_count_grid("PCGX_SHAPES_SPLIT", n_hyp, n, &chunk);
  const unsigned fit_blocks = (unsigned)((n_hyp + 255) / 256);
  const ShapeState *S = b.S;
  const float4 *Pc = Pid, *Nc = Nid;
  return peel_rounds<ShapeModel>(
      b, (int32_t)n, n_hyp, max_shapes, min_inliers, refine, T, left, o, st,
      [&](const PeelRound &q) {
        const uint32_t *smp = d_samples + 2 * n_hyp * q.r;
        const int32_t *pt = partner;
        if (local) {
          if (src == kRangeXWalk)
            partner_launch<kRangeXWalk>(t, tv, xv, stack_bytes, S, q.A, q.P, smp, n_hyp, bound, left, partner, st);
          else if (src == kRangeGrid)
            partner_launch<kRangeGrid>(t, tv, xv, stack_bytes, S, q.A, q.P, smp, n_hyp, bound, left, partner, st);
          else
            partner_launch<kRangeWalk>(t, tv, xv, stack_bytes, S, q.A, q.P, smp, n_hyp, bound, left, partner, st);
        }
        hipLaunchKernelGGL(shapes_fit_kernel, dim3(fit_blocks), dim3(256), 0, st, S, q.A, Pc, Nc, smp, pt, n_hyp, kind, ax,
                           r_min, r_max, q.status, q.counts, q.hyp);
        const float md = max_dist, c2 = T.c2;
        if (kind == kShapeSphere) {
          if (normal_test)
            count_launch<kShapeSphere, true>(count_grid, S, q.P, q.N, n_hyp, q.status, q.hyp, md, c2, chunk, q.counts, st);
          else
            count_launch<kShapeSphere, false>(count_grid, S, q.P, q.N, n_hyp, q.status, q.hyp, md, c2, chunk, q.counts, st);
        } else {
          if (normal_test)
            count_launch<kShapeCylinder, true>(count_grid, S, q.P, q.N, n_hyp, q.status, q.hyp, md, c2, chunk, q.counts, st);
          else
            count_launch<kShapeCylinder, false>(count_grid, S, q.P, q.N, n_hyp, q.status, q.hyp, md, c2, chunk, q.counts, st);
        }
      },
      [&](const PeelRound &) -> pcgx_status {
        const int32_t *cand = b.cand;
        const double *sums = partial;
        hipLaunchKernelGGL(shapes_sums_kernel, dim3(b.tiles), dim3(kScBlock), 0, st, S, kind, cand, Pc, partial);
        hipLaunchKernelGGL(shapes_refit_kernel, dim3(1), dim3(64), 0, st, b.S, kind, sums, r_min, r_max);
        return PCGX_OK;
      });
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
  if (!n_shapes || !shapes || !sizes || !refined || !best || (t->n > 0 && !labels))
    return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  return peel_host<ShapeModel::kRec>(
      t->n, 2, samples, n_hyp, max_shapes, normals, n_shapes, shapes, sizes, refined, best, labels, ids, status, counts,
      hyp_shapes, [&](const uint32_t *d_samples, const float *d_normals, const PeelOut &d, hipStream_t st) {
        return pcgx_kdtree_shapes_dev(t, kind, d_samples, n_hyp, max_shapes, max_dist, min_inliers, sample_radius, r_min,
                                      r_max, axis, min_axis_cos, d_normals, min_normal_cos, refine, d.n_found, d.recs, d.sizes,
                                      d.refined, d.best, d.labels, d.ids, d.status, d.counts, d.hyp, st);
      });
}
