// fpfh.hip -- Fast Point Feature Histograms (Rusu, Blodow, Beetz 2009) of a tree's own points over radius
// neighbourhoods and caller-given normals (extension: no reference parity; include/pcgx.h, "FPFH descriptors").
//
// The input of feature-based coarse alignment, the step before every ICP here.  Two kernels over the enumeration that
// Range, normals and region growing share (radius_visit.h), one query per lane, the queries the tree's own points as
// query_source lays them out, on each of the three kinds of handle (grid, forced walk, patched tree after DeletePoint):
//   spfh_kernel  per neighbour: its normal by id, the pair's three bins (fpfh_terms.h), three 32-bit counters of the
//                lane's column of an LDS table [34][64] (the bin index is dynamic: registers indexed by it would go to
//                scratch; row 33 counts the valid pairs).  Writes one record per point: {c[33], m, 0, 0}, 36 uint32.
//   fpfh_kernel  the same enumeration again; per neighbour with DistSq > 0: its record by id as nine uint4 and
//                (1 / DistSq) / m_i times its counts into 33 float64 accumulators (constant indices: registers).  Then
//                F = 100 c_q / m_q + 100 W / T_f per feature, rounded to float32.
// The record keeps the COUNTS, not 100 c / m rounded to float32: the same 144 bytes, one division per neighbour
// instead of none, and the sums are then those of the contract's real numbers to float64 rounding -- a bin nobody
// counted is exactly 0, and the factor 100 cancels in W / T.
// Of a fat row's shares, in both kernels: the counts go into the owner's LDS column by LDS atomics (integers: any order
// gives the same bits), the float64 partials are summed by shuffles.
//
// Descriptors at chosen ids only (pcgx_kdtree_fpfh_at, include/pcgx.h "FPFH at chosen points"): three stages over the
// same enumeration; the queries of the first and the third are the selected points, fetched by id, one slot per lane:
//   fpfh_mark_kernel         a 1 into need[j] for the slot's point and for every member of its N(.) (plain byte stores
//                            of one value: no atomics, any order), the slot's xyz, and a dead slot's zeros.
//   spfh_kernel<., true>     over the tree's own points in cell order; a lane whose need byte is 0 enumerates nothing
//                            and writes no record (local_maxima_kernel's way with a score that cannot qualify).  The
//                            flags are then counted by bucket_grid.h's tile count and one scan workgroup.
//   fpfh_kernel<., true>     the query a live slot's point, the row written at the slot.  A lane's sums run over its
//                            query's neighbourhood in the order the every-point form's lane takes for that point (the
//                            rows of the grid as grid_cover names them, a walk from the root): the same row, bit for bit.
// Each pair is one kernel template, the form a compile-time bool; what that did to the every-point instantiations'
// resources and times is DESIGN.md 3.6.1.
#include <math.h>
#include <stdlib.h>

#include <type_traits>

#include "bucket_grid.h"
#include "fpfh_terms.h"
#include "radius_visit.h"

namespace pcgx {

constexpr int kFpfhBlock = kRangeWalkBlock;  // one wave per workgroup: the walks' LDS frame stacks are [level][64]
constexpr int kFpfhRows = kFpfhLen + 1;      // the LDS table's rows: 33 bins and the valid pairs
constexpr int kFpfhRec = 36;                 // uint32 per record: c[33], m, 0, 0 -- nine uint4
static_assert(kFpfhBlock == 64, "one wave: a lane's LDS column is [row][lane]");
static_assert(kFpfhRec % 4 == 0 && kFpfhRec >= kFpfhRows, "whole uint4s");

struct SpfhOut {
  const float *normals;  // [3 n], id order
  uint4 *rec;            // [9 n]
  int32_t *counts;       // [33 n] or nullptr
  int32_t *pairs;        // [n] or nullptr
  const uint8_t *need;   // [n], kNeed only: a record where the byte is set, the others stay unwritten and unread
};

// the pair (query s of column col, neighbour p) into the column's counters
__device__ __forceinline__ void spfh_pair(uint32_t *cnt, const int col, const float *normals, const float4 &p,
                                          const float sx, const float sy, const float sz, const float nx,
                                          const float ny, const float nz) {
  const size_t id = (size_t)__float_as_uint(p.w);
  int b1, b2, b3;
  if (!fpfh_terms(sx, sy, sz, nx, ny, nz, p.x, p.y, p.z, normals[3 * id], normals[3 * id + 1], normals[3 * id + 2], b1,
                  b2, b3))
    return;
  atomicAdd(&cnt[b1 * kFpfhBlock + col], 1u);
  atomicAdd(&cnt[(kFpfhBins + b2) * kFpfhBlock + col], 1u);
  atomicAdd(&cnt[(2 * kFpfhBins + b3) * kFpfhBlock + col], 1u);
  atomicAdd(&cnt[kFpfhLen * kFpfhBlock + col], 1u);
}

// kNeed: only the points whose need byte is set (FPFH at chosen points); else every point
template <int kSrc, bool kNeed>
__global__ __launch_bounds__(kFpfhBlock) void spfh_kernel(GridView g, TreeView tv, XTreeView xv, QuerySource Q,
                                                          float bound, SpfhOut O, int64_t guard) {
  extern __shared__ uint32_t s_stack[];
  __shared__ uint32_t s_cnt[kFpfhRows * kFpfhBlock];
  const uint32_t n_tiles = (uint32_t)((Q.nq + kFpfhBlock - 1) / kFpfhBlock);
  const int64_t pos = (int64_t)xcd_tile(blockIdx.x, n_tiles) * kFpfhBlock + threadIdx.x;
  const int lane = (int)threadIdx.x;
#pragma unroll
  for (int k = 0; k < kFpfhRows; k++) s_cnt[k * kFpfhBlock + lane] = 0u;
  bool live = pos < Q.nq;
  int64_t i = 0;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (live) {
    read_query(Q, pos, i, qx, qy, qz);
    if constexpr (kNeed) live = O.need[i] != 0;
  }
  if (live) {
    nx = O.normals[3 * i];
    ny = O.normals[3 * i + 1];
    nz = O.normals[3 * i + 2];
  }
  // (one wave: the zeroes are in place before another lane's atomics land in this column)
  if constexpr (kSrc == kRangeGrid) __syncthreads();
  radius_visit<kSrc>(
      RadiusViews{g, tv, xv, guard}, s_stack + threadIdx.x, kFpfhBlock, qx, qy, qz, bound, live,
      [&](const float4 &p, float) { spfh_pair(s_cnt, lane, O.normals, p, qx, qy, qz, nx, ny, nz); },
      [&](int owner, float ox, float oy, float oz, auto rows) {
        const float onx = __shfl(nx, owner), ony = __shfl(ny, owner), onz = __shfl(nz, owner);
        rows([&](const float4 &p, float) { spfh_pair(s_cnt, owner, O.normals, p, ox, oy, oz, onx, ony, onz); });
      });
  if constexpr (kSrc == kRangeGrid) __syncthreads();  // the other lanes' atomics before the owner reads its column
  if (!live) return;
  uint32_t c[kFpfhRec];
#pragma unroll
  for (int k = 0; k < kFpfhRec; k++) c[k] = k < kFpfhRows ? s_cnt[k * kFpfhBlock + lane] : 0u;
#pragma unroll
  for (int k = 0; k < kFpfhRec / 4; k++) O.rec[(kFpfhRec / 4) * i + k] = make_uint4(c[4 * k], c[4 * k + 1], c[4 * k + 2], c[4 * k + 3]);
  if (O.counts) {
#pragma unroll
    for (int k = 0; k < kFpfhLen; k++) O.counts[kFpfhLen * i + k] = (int32_t)c[k];
  }
  if (O.pairs) O.pairs[i] = (int32_t)c[kFpfhLen];
}

// sum over the neighbours of (1 / DistSq) c_i / m_i, bin by bin
struct FpfhAcc {
  double a[kFpfhLen];

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < kFpfhLen; k++) a[k] = 0.0;
  }
  // neighbour p at float32 DistSq d of the query
  __device__ __forceinline__ void add(const uint4 *rec, const float4 &p, const float d) {
    if (d == 0.0f) return;  // the point itself and its duplicates
    const uint4 *r = rec + (size_t)(kFpfhRec / 4) * (size_t)__float_as_uint(p.w);
    uint4 q[kFpfhRec / 4];
#pragma unroll
    for (int k = 0; k < kFpfhRec / 4; k++) q[k] = r[k];
    const uint32_t m = q[kFpfhLen / 4].y;  // word 33
    if (m == 0u) return;                   // S_i = 0
    const double wm = (1.0 / (double)d) / (double)m;
#pragma unroll
    for (int k = 0; k < kFpfhLen; k++) {
      const uint4 &u = q[k / 4];
      const uint32_t ck = k % 4 == 0 ? u.x : (k % 4 == 1 ? u.y : (k % 4 == 2 ? u.z : u.w));
      a[k] = fma(wm, (double)ck, a[k]);
    }
  }
  // the whole wave's partials into every lane (all 64 lanes must be here)
  __device__ __forceinline__ void wave_sum() {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
      for (int k = 0; k < kFpfhLen; k++) a[k] += __shfl_xor(a[k], m);
    }
  }
  __device__ __forceinline__ void merge(const FpfhAcc &o) {
#pragma unroll
    for (int k = 0; k < kFpfhLen; k++) a[k] += o.a[k];
  }
};

// ---- descriptors at chosen ids: where the queries come from and where the rows go

// the slots: ids[cap], of which the first clamp(*n_ids, 0, cap) count (n_ids == nullptr: all), and where a point's
// xyz is found by id
struct FpfhSlots {
  const int32_t *ids;
  const int32_t *n_ids;
  int32_t cap;
  int64_t n;            // Len()
  const uint32_t *inv;  // grid, walk: id -> BFS slot of its node in the implicit tree (range_inverse_map)
  const float *xyz;     // patched tree: the cloud's points by id (t->d_xsrc)
};

// slot s: live?  Then its point id i and the point.
template <int kSrc>
__device__ __forceinline__ bool read_slot(const FpfhSlots &S, const TreeView &tv, const int64_t s, int64_t &i, float &qx,
                                          float &qy, float &qz) {
  if (s >= (int64_t)S.cap) return false;
  if (S.n_ids && s >= (int64_t)*S.n_ids) return false;  // (a negative count: no slot is below it)
  const int32_t id = S.ids[s];
  if (id < 0 || (int64_t)id >= S.n) return false;
  i = (int64_t)id;
  if constexpr (kSrc == kRangeXWalk) {
    qx = S.xyz[3 * i];
    qy = S.xyz[3 * i + 1];
    qz = S.xyz[3 * i + 2];
  } else {
    const float4 nd = node_at(tv.nodes, S.inv[i]);
    qx = nd.x;
    qy = nd.y;
    qz = nd.z;
  }
  return true;
}

struct FpfhAtOut {
  float *fpfh;      // [33 cap]
  float *xyz;       // [3 cap] or nullptr
  int32_t *counts;  // [33 cap] or nullptr
  int32_t *pairs;   // [cap] or nullptr
};

// kAt: a query per slot, the live slot's point, and the row, the point's counts and its pairs written at the slot;
// else the tree's own points as query_source lays them out, the row (O.fpfh alone) at the point's id
template <int kSrc, bool kAt>
__global__ __launch_bounds__(kFpfhBlock) void fpfh_kernel(GridView g, TreeView tv, XTreeView xv,
                                                          std::conditional_t<kAt, FpfhSlots, QuerySource> Q, float bound,
                                                          const uint4 *rec, FpfhAtOut O, int64_t guard) {
  extern __shared__ uint32_t s_stack[];
  int64_t i = 0, row = 0;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  bool live;
  if constexpr (kAt) {
    row = (int64_t)blockIdx.x * kFpfhBlock + threadIdx.x;
    live = read_slot<kSrc>(Q, tv, row, i, qx, qy, qz);
  } else {
    const uint32_t n_tiles = (uint32_t)((Q.nq + kFpfhBlock - 1) / kFpfhBlock);
    const int64_t pos = (int64_t)xcd_tile(blockIdx.x, n_tiles) * kFpfhBlock + threadIdx.x;
    live = pos < Q.nq;
    if (live) read_query(Q, pos, i, qx, qy, qz);
    row = i;
  }
  const int lane = (int)(threadIdx.x & 63u);
  FpfhAcc acc;
  acc.clear();
  radius_visit<kSrc>(
      RadiusViews{g, tv, xv, guard}, s_stack + threadIdx.x, kFpfhBlock, qx, qy, qz, bound, live,
      [&](const float4 &p, float d) { acc.add(rec, p, d); },
      [&](int owner, float, float, float, auto rows) {
        FpfhAcc part;
        part.clear();
        rows([&](const float4 &p, float d) { part.add(rec, p, d); });
        part.wave_sum();
        if (lane == owner) acc.merge(part);
      });
  if (!live) return;
  // F = S_q + 100 W / T per feature
  const uint4 *own = rec + (size_t)(kFpfhRec / 4) * (size_t)i;
  uint4 q[kFpfhRec / 4];
#pragma unroll
  for (int k = 0; k < kFpfhRec / 4; k++) q[k] = own[k];
  const uint32_t m = q[kFpfhLen / 4].y;
  const double sq = m ? 100.0 / (double)m : 0.0;
#pragma unroll
  for (int f = 0; f < 3; f++) {
    double T = 0.0;
#pragma unroll
    for (int b = 0; b < kFpfhBins; b++) T += acc.a[f * kFpfhBins + b];
    const double sc = T > 0.0 ? 100.0 / T : 0.0;
#pragma unroll
    for (int b = 0; b < kFpfhBins; b++) {
      const int k = f * kFpfhBins + b;
      const uint4 &u = q[k / 4];
      const uint32_t ck = k % 4 == 0 ? u.x : (k % 4 == 1 ? u.y : (k % 4 == 2 ? u.z : u.w));
      O.fpfh[(size_t)kFpfhLen * (size_t)row + k] = (float)((double)ck * sq + acc.a[k] * sc);
      if constexpr (kAt) {
        if (O.counts) O.counts[(size_t)kFpfhLen * (size_t)row + k] = (int32_t)ck;
      }
    }
  }
  if constexpr (kAt) {
    if (O.pairs) O.pairs[row] = (int32_t)m;
  }
}

template <int kSrc>
__global__ __launch_bounds__(kFpfhBlock) void fpfh_mark_kernel(GridView g, TreeView tv, XTreeView xv, FpfhSlots S,
                                                               float bound, uint8_t *__restrict__ need, FpfhAtOut O,
                                                               int64_t guard) {
  extern __shared__ uint32_t s_stack[];
  const int64_t s = (int64_t)blockIdx.x * kFpfhBlock + threadIdx.x;
  int64_t i = 0;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  const bool live = read_slot<kSrc>(S, tv, s, i, qx, qy, qz);
  if (s < (int64_t)S.cap) {
    if (O.xyz) {
      O.xyz[3 * s] = qx;
      O.xyz[3 * s + 1] = qy;
      O.xyz[3 * s + 2] = qz;
    }
    if (!live) {  // a dead slot: zeros (fpfh_kernel<., true> writes the live ones)
      for (int k = 0; k < kFpfhLen; k++) {
        O.fpfh[(size_t)kFpfhLen * (size_t)s + k] = 0.0f;
        if (O.counts) O.counts[(size_t)kFpfhLen * (size_t)s + k] = 0;
      }
      if (O.pairs) O.pairs[s] = 0;
    }
  }
  if (live) need[i] = (uint8_t)1;  // (a deleted id, a NaN coordinate: the point does not meet itself)
  auto mark = [&](const float4 &p, float) { need[__float_as_uint(p.w)] = (uint8_t)1; };
  radius_visit<kSrc>(RadiusViews{g, tv, xv, guard}, s_stack + threadIdx.x, kFpfhBlock, qx, qy, qz, bound, live, mark,
                     [&](int, float, float, float, auto rows) { rows(mark); });
}

__global__ __launch_bounds__(256) void fpfh_need_count_kernel(const uint8_t *__restrict__ need, int64_t n,
                                                              uint32_t *__restrict__ tile_count) {
  tile_flag_count(n, [&](int64_t j) { return need[j] != 0; }, tile_count);
}
__global__ __launch_bounds__(1024) void fpfh_need_scan_kernel(uint32_t *__restrict__ tile_count, int ntiles,
                                                              uint32_t *__restrict__ total) {
  tile_scan(tile_count, ntiles, total);
}

}  // namespace pcgx

using namespace pcgx;

namespace {

pcgx_status fpfh_check(const char *fn, const pcgx_kdtree *t, const float *normals, float radius, const float *fpfh) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!(radius > 0.0f) || !(radius < __builtin_inff())) return fail(PCGX_E_INVALID, "%s: radius must be finite and > 0", fn);
  if (t->n > 0 && !normals) return fail(PCGX_E_INVALID, "%s: NULL normals", fn);
  if (t->n > 0 && !fpfh) return fail(PCGX_E_INVALID, "%s: NULL fpfh", fn);
  return PCGX_OK;
}

template <int kSrc>
void fpfh_launch(const pcgx_kdtree *t, const TreeView &tv, const XTreeView &xv, const QuerySource &Q, float bound,
                 const SpfhOut &O, float *d_fpfh, size_t stack_bytes, hipStream_t st) {
  const dim3 grid(xcd_grid((unsigned)((Q.nq + kFpfhBlock - 1) / kFpfhBlock))), block(kFpfhBlock);
  const int64_t guard = xwalk_guard(t->n);
  const GridView g = kSrc == kRangeGrid ? t->grid : GridView{};
  hipLaunchKernelGGL((spfh_kernel<kSrc, false>), grid, block, stack_bytes, st, g, tv, xv, Q, bound, O, guard);
  hipLaunchKernelGGL((fpfh_kernel<kSrc, false>), grid, block, stack_bytes, st, g, tv, xv, Q, bound, (const uint4 *)O.rec,
                     FpfhAtOut{d_fpfh, nullptr, nullptr, nullptr}, guard);
}

// everything device resident; the SPFH records and the queries from ctx().arena
pcgx_status fpfh_enqueue(const pcgx_kdtree *t, const float *d_normals, float radius, float *d_fpfh, int32_t *d_counts,
                         int32_t *d_pairs, hipStream_t st) {
  PCGX_TRY(ctx().arena.begin(st));
  const RangeSrc src = range_source(t);  // as pcgx_kdtree_range_count takes it
  XTreeView xv{};
  if (src == kRangeXWalk) PCGX_TRY(xtree_view(t, &xv, st));
  const TreeView tv = t->view();
  QuerySource Q;
  PCGX_TRY(query_source(t, src, nullptr, t->n, &Q, st));
  SpfhOut O{d_normals, nullptr, d_counts, d_pairs, nullptr};
  PCGX_TRY(ctx().arena.alloc_n((size_t)t->n * (kFpfhRec / 4), &O.rec));
  const float bound = radius * radius;
  if (src == kRangeXWalk) fpfh_launch<kRangeXWalk>(t, tv, xv, Q, bound, O, d_fpfh, xwalk_stack_bytes(xv, kFpfhBlock), st);
  else if (src == kRangeGrid) fpfh_launch<kRangeGrid>(t, tv, xv, Q, bound, O, d_fpfh, 0, st);
  else fpfh_launch<kRangeWalk>(t, tv, xv, Q, bound, O, d_fpfh, walk_stack_bytes(tv, kFpfhBlock), st);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

constexpr int64_t kFpfhAtMax = 0x7fffffff;  // ids and counts are int32 on the device

pcgx_status fpfh_at_check(const char *fn, const pcgx_kdtree *t, const float *normals, float radius, const void *ids,
                          int64_t count, const float *fpfh) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!(radius > 0.0f) || !(radius < __builtin_inff())) return fail(PCGX_E_INVALID, "%s: radius must be finite and > 0", fn);
  if (count < 0) return fail(PCGX_E_INVALID, "%s: negative number of ids", fn);
  if (count > kFpfhAtMax || t->n > kFpfhAtMax) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 ids or points", fn);
  if (count > 0 && !ids) return fail(PCGX_E_INVALID, "%s: NULL ids", fn);
  if (count > 0 && !fpfh) return fail(PCGX_E_INVALID, "%s: NULL fpfh", fn);
  if (count > 0 && t->n > 0 && !normals) return fail(PCGX_E_INVALID, "%s: NULL normals", fn);
  return PCGX_OK;
}

template <int kSrc>
void fpfh_at_launch(const pcgx_kdtree *t, const TreeView &tv, const XTreeView &xv, const QuerySource &Q,
                    const FpfhSlots &S, float bound, const float *d_normals, uint8_t *d_need, uint4 *d_rec,
                    const FpfhAtOut &O, size_t stack_bytes, hipStream_t st) {
  const dim3 slots((unsigned)(((int64_t)S.cap + kFpfhBlock - 1) / kFpfhBlock));
  const dim3 points(xcd_grid((unsigned)((Q.nq + kFpfhBlock - 1) / kFpfhBlock))), block(kFpfhBlock);
  const int64_t guard = xwalk_guard(t->n);
  const GridView g = kSrc == kRangeGrid ? t->grid : GridView{};
  hipLaunchKernelGGL(fpfh_mark_kernel<kSrc>, slots, block, stack_bytes, st, g, tv, xv, S, bound, d_need, O, guard);
  hipLaunchKernelGGL((spfh_kernel<kSrc, true>), points, block, stack_bytes, st, g, tv, xv, Q, bound,
                     SpfhOut{d_normals, d_rec, nullptr, nullptr, d_need}, guard);
  hipLaunchKernelGGL((fpfh_kernel<kSrc, true>), slots, block, stack_bytes, st, g, tv, xv, S, bound, (const uint4 *)d_rec,
                     O, guard);
}

// Len() > 0, cap > 0, everything device resident; the flags, the SPFH records and the tile counts from ctx().arena
pcgx_status fpfh_at_enqueue(const pcgx_kdtree *t, const float *d_normals, float radius, const int32_t *d_ids, int64_t cap,
                            const int32_t *d_n_ids, const FpfhAtOut &O, int32_t *d_n_spfh, hipStream_t st) {
  PCGX_TRY(ctx().arena.begin(st));
  const int64_t n = t->n;
  const RangeSrc src = range_source(t);  // as pcgx_kdtree_range_count takes it
  XTreeView xv{};
  if (src == kRangeXWalk) PCGX_TRY(xtree_view(t, &xv, st));
  FpfhSlots S{d_ids, d_n_ids, (int32_t)cap, n, nullptr, nullptr};  // (xtree_view made d_xsrc)
  if (src == kRangeXWalk) S.xyz = t->d_xsrc;
  else PCGX_TRY(range_inverse_map(t, &S.inv, st));
  const TreeView tv = t->view();
  QuerySource Q;
  PCGX_TRY(query_source(t, src, nullptr, n, &Q, st));
  uint8_t *d_need = nullptr;
  uint4 *d_rec = nullptr;
  PCGX_TRY(ctx().arena.alloc_n((size_t)n, &d_need));
  PCGX_TRY(ctx().arena.alloc_n((size_t)n * (kFpfhRec / 4), &d_rec));
  // (the arena hands out what an earlier call used: the flags start from zero on every call)
  PCGX_HIP_TRY(hipMemsetAsync(d_need, 0, (size_t)n, st));
  const float bound = radius * radius;
  if (src == kRangeXWalk)
    fpfh_at_launch<kRangeXWalk>(t, tv, xv, Q, S, bound, d_normals, d_need, d_rec, O, xwalk_stack_bytes(xv, kFpfhBlock), st);
  else if (src == kRangeGrid) fpfh_at_launch<kRangeGrid>(t, tv, xv, Q, S, bound, d_normals, d_need, d_rec, O, 0, st);
  else fpfh_at_launch<kRangeWalk>(t, tv, xv, Q, S, bound, d_normals, d_need, d_rec, O, walk_stack_bytes(tv, kFpfhBlock), st);
  if (d_n_spfh) {
    const int ntiles = (int)((n + kRunTile - 1) / kRunTile);
    uint32_t *tile_count = nullptr;
    PCGX_TRY(ctx().arena.alloc_n((size_t)ntiles, &tile_count));
    hipLaunchKernelGGL(fpfh_need_count_kernel, dim3(ntiles), dim3(256), 0, st, (const uint8_t *)d_need, n, tile_count);
    hipLaunchKernelGGL(fpfh_need_scan_kernel, dim3(1), dim3(1024), 0, st, tile_count, ntiles, (uint32_t *)d_n_spfh);
  }
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

}  // namespace

extern "C" pcgx_status pcgx_kdtree_fpfh_at_dev(const pcgx_kdtree *t, const float *d_normals, float radius,
                                               const int32_t *d_ids, int64_t cap, const int32_t *d_n_ids, float *d_fpfh,
                                               float *d_xyz, int32_t *d_spfh_counts, int32_t *d_pair_counts,
                                               int32_t *d_n_spfh, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(fpfh_at_check("pcgx_kdtree_fpfh_at_dev", t, d_normals, radius, d_ids, cap, d_fpfh));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  if (t->n == 0 || cap == 0) {  // no point to describe: every slot is dead
    const size_t c = (size_t)cap;
    if (d_n_spfh) PCGX_HIP_TRY(hipMemsetAsync(d_n_spfh, 0, sizeof(int32_t), st));
    if (c == 0) return PCGX_OK;
    PCGX_HIP_TRY(hipMemsetAsync(d_fpfh, 0, c * kFpfhLen * 4, st));
    if (d_xyz) PCGX_HIP_TRY(hipMemsetAsync(d_xyz, 0, c * 12, st));
    if (d_spfh_counts) PCGX_HIP_TRY(hipMemsetAsync(d_spfh_counts, 0, c * kFpfhLen * 4, st));
    if (d_pair_counts) PCGX_HIP_TRY(hipMemsetAsync(d_pair_counts, 0, c * 4, st));
    return PCGX_OK;
  }
  return fpfh_at_enqueue(t, d_normals, radius, d_ids, cap, d_n_ids, FpfhAtOut{d_fpfh, d_xyz, d_spfh_counts, d_pair_counts},
                         d_n_spfh, st);
}

extern "C" pcgx_status pcgx_kdtree_fpfh_at(const pcgx_kdtree *t, const float *normals, float radius, const int64_t *ids,
                                           int64_t n_ids, float *fpfh, float *xyz, int32_t *spfh_counts,
                                           int32_t *pair_counts, int64_t *n_spfh) {
  PCGX_API_CALL();
  PCGX_TRY(fpfh_at_check("pcgx_kdtree_fpfh_at", t, normals, radius, ids, n_ids, fpfh));
  if (n_spfh) *n_spfh = 0;
  if (n_ids == 0) return PCGX_OK;
  const int64_t n = t->n;
  RawVector<int32_t> h((size_t)n_ids + 1);  // the ids, and the record count coming back
  for (int64_t s = 0; s < n_ids; s++) {
    if (ids[s] < 0 || ids[s] >= n) return fail(PCGX_E_INVALID, "pcgx_kdtree_fpfh_at: id out of range");
    h[(size_t)s] = (int32_t)ids[s];
  }
  PCGX_TRY(ensure_init());
  // always on the device: the bins and the sums are the kernels', not a host restatement
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_n = nullptr, *d_f = nullptr, *d_x = nullptr;
  int32_t *d_i = nullptr, *d_c = nullptr, *d_m = nullptr;  // d_i: ids [n_ids], the record count
  PCGX_TRY(ha.alloc_n((size_t)n * 3, &d_n));
  PCGX_TRY(staged_upload(d_n, normals, (size_t)n * 12, st));
  PCGX_TRY(ha.alloc_n((size_t)n_ids + 1, &d_i));
  PCGX_TRY(staged_upload(d_i, h.data(), (size_t)n_ids * 4, st));
  PCGX_TRY(ha.alloc_n((size_t)n_ids * kFpfhLen, &d_f));
  if (xyz) PCGX_TRY(ha.alloc_n((size_t)n_ids * 3, &d_x));
  if (spfh_counts) PCGX_TRY(ha.alloc_n((size_t)n_ids * kFpfhLen, &d_c));
  if (pair_counts) PCGX_TRY(ha.alloc_n((size_t)n_ids, &d_m));
  PCGX_TRY(pcgx_kdtree_fpfh_at_dev(t, d_n, radius, d_i, n_ids, nullptr, d_f, d_x, d_c, d_m, d_i + n_ids, st));
  PCGX_TRY(staged_download(fpfh, d_f, (size_t)n_ids * kFpfhLen * 4, st));
  if (xyz) PCGX_TRY(staged_download(xyz, d_x, (size_t)n_ids * 12, st));
  if (spfh_counts) PCGX_TRY(staged_download(spfh_counts, d_c, (size_t)n_ids * kFpfhLen * 4, st));
  if (pair_counts) PCGX_TRY(staged_download(pair_counts, d_m, (size_t)n_ids * 4, st));
  if (n_spfh) {
    int32_t c = 0;
    PCGX_TRY(staged_download(&c, d_i + n_ids, 4, st));
    *n_spfh = c;
  }
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_kdtree_fpfh_dev(const pcgx_kdtree *t, const float *d_normals, float radius, float *d_fpfh,
                                            int32_t *d_spfh_counts, int32_t *d_pair_counts, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(fpfh_check("pcgx_kdtree_fpfh_dev", t, d_normals, radius, d_fpfh));
  if (t->n == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  return fpfh_enqueue(t, d_normals, radius, d_fpfh, d_spfh_counts, d_pair_counts, pick_stream(stream));
}

extern "C" pcgx_status pcgx_kdtree_fpfh(const pcgx_kdtree *t, const float *normals, float radius, float *fpfh,
                                        int32_t *spfh_counts, int32_t *pair_counts) {
  PCGX_API_CALL();
  PCGX_TRY(fpfh_check("pcgx_kdtree_fpfh", t, normals, radius, fpfh));
  const int64_t n = t->n;
  if (n == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  // always on the device: the bins and the sums are the kernels', not a host restatement
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_n = nullptr, *d_f = nullptr;
  int32_t *d_c = nullptr, *d_m = nullptr;
  PCGX_TRY(ha.alloc_n((size_t)n * 3, &d_n));
  PCGX_TRY(staged_upload(d_n, normals, (size_t)n * 12, st));
  PCGX_TRY(ha.alloc_n((size_t)n * kFpfhLen, &d_f));
  if (spfh_counts) PCGX_TRY(ha.alloc_n((size_t)n * kFpfhLen, &d_c));
  if (pair_counts) PCGX_TRY(ha.alloc_n((size_t)n, &d_m));
  PCGX_TRY(pcgx_kdtree_fpfh_dev(t, d_n, radius, d_f, d_c, d_m, st));
  PCGX_TRY(staged_download(fpfh, d_f, (size_t)n * kFpfhLen * 4, st));
  if (spfh_counts) PCGX_TRY(staged_download(spfh_counts, d_c, (size_t)n * kFpfhLen * 4, st));
  if (pair_counts) PCGX_TRY(staged_download(pair_counts, d_m, (size_t)n * 4, st));
  return PCGX_OK;
}
