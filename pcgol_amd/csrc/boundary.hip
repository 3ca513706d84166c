// boundary.hip -- boundary points of a cloud: the points whose neighbours leave a wide angular gap in the tangent plane
// (extension: no reference parity; include/pcgx.h, "boundary points").
//
// What the closed-surface stages do not say: where a scan ends -- the rim of a partial view, the shadow behind an
// object, a hole.  One operation over a tree's own points, as query_source lays them out, on each of the three kinds of
// handle (grid, forced walk, patched tree after DeletePoint):
//   boundary_kernel   a consumer of the shared enumeration (radius_visit.h), one query per lane.  A lane reads its own
//                     normal by id once and builds the tangent frame in registers (boundary_terms.h); a lane whose
//                     normal gives no frame enumerates nothing.  Per record inside the bound: its direction in the frame
//                     (float64, about twenty operations), one of 64 sectors, one bit ORed into the lane's mask, one added
//                     to its count, and "met myself" (a deleted id or a NaN coordinate never meets itself).  The record
//                     carries the position: nothing is gathered by id.  Then the longest cyclic run of zero bits, one
//                     flag byte per id and the optional gaps, masks and counts.
//   compaction        the flags to ascending ids and the -1 tail by keypoints.hip's four launches.
// Of a fat row's shares the masks are ORed and the counts added over the wave by shuffles of 32-bit words, "met myself"
// by a ballot, and the owner merges them.  OR and + commute: the result is a property of the point set, not of the
// order of the visit.
#include <math.h>
#include <stdlib.h>

#include "boundary_terms.h"
#include "bucket_grid.h"
#include "radius_visit.h"

namespace pcgx {

// keypoints.hip
pcgx_status flags_to_ids_enqueue(const uint8_t *d_flag, int64_t n, uint32_t *tile_count, int32_t *d_ids, int32_t *d_n_ids,
                                 hipStream_t st);

constexpr int kBoundaryBlock = kRangeWalkBlock;  // one wave per workgroup: the walks' LDS frame stacks are [level][64]

// the state of one query
struct BoundaryBits {
  uint64_t mask;
  int32_t count;
  bool met;

  // the record p, inside the bound of query i at (qx, qy, qz) with the frame f
  __device__ __forceinline__ void take(const BoundaryFrame &f, const float4 &p, const float qx, const float qy,
                                       const float qz, const int32_t i) {
    met = met || (int32_t)__float_as_uint(p.w) == i;
    count++;
    double a, b;
    boundary_direction(f, p.x, p.y, p.z, qx, qy, qz, a, b);
    const int s = boundary_sector(a, b);
    if (s >= 0) mask |= (uint64_t)1 << s;
  }
};

struct BoundaryOut {
  uint8_t *flag;    // [Len()]
  int32_t *gaps;    // [Len()] or NULL
  uint64_t *masks;  // [Len()] or NULL
  int32_t *counts;  // [Len()] or NULL
};

template <int kSrc>
__global__ __launch_bounds__(kBoundaryBlock) void boundary_kernel(GridView g, TreeView tv, XTreeView xv, QuerySource Q,
                                                                  float bound, const float *__restrict__ normals,
                                                                  int32_t min_gap, int32_t min_neighbors, BoundaryOut out,
                                                                  int64_t guard) {
  extern __shared__ uint32_t s_stack[];
  const uint32_t n_tiles = (uint32_t)((Q.nq + kBoundaryBlock - 1) / kBoundaryBlock);
  const int64_t pos = (int64_t)xcd_tile(blockIdx.x, n_tiles) * kBoundaryBlock + threadIdx.x;
  const bool live = pos < Q.nq;
  int64_t i64 = 0;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (live) {
    read_query(Q, pos, i64, qx, qy, qz);
    nx = normals[3 * i64], ny = normals[3 * i64 + 1], nz = normals[3 * i64 + 2];
  }
  const int32_t i = (int32_t)i64;
  const bool usable = live && boundary_normal_usable(nx, ny, nz);  // nothing to enumerate without a frame
  const BoundaryFrame f = boundary_frame(nx, ny, nz);
  BoundaryBits b{0ull, 0, false};
  const int lane = (int)(threadIdx.x & 63u);
  radius_visit<kSrc>(
      RadiusViews{g, tv, xv, guard}, s_stack + threadIdx.x, kBoundaryBlock, qx, qy, qz, bound, usable,
      [&](const float4 &p, float) { b.take(f, p, qx, qy, qz, i); },
      [&](int owner, float ox, float oy, float oz, auto rows) {  // the owner's frame again from its normal: three words
        const BoundaryFrame of = boundary_frame(__shfl(nx, owner), __shfl(ny, owner), __shfl(nz, owner));
        const int32_t oi = __shfl(i, owner);
        BoundaryBits part{0ull, 0, false};
        rows([&](const float4 &p, float) { part.take(of, p, ox, oy, oz, oi); });
        uint32_t lo = (uint32_t)part.mask, hi = (uint32_t)(part.mask >> 32);
        int32_t c = part.count;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
          lo |= __shfl_xor(lo, m);
          hi |= __shfl_xor(hi, m);
          c += __shfl_xor(c, m);
        }
        const bool any_met = __ballot(part.met) != 0ull;
        if (lane == owner) {
          b.mask |= ((uint64_t)hi << 32) | (uint64_t)lo;
          b.count += c;
          b.met = b.met || any_met;
        }
      });
  if (!live) return;
  const bool evaluated = boundary_evaluated(b.met, usable, b.count, min_neighbors);
  const uint64_t mask = evaluated ? b.mask : 0ull;
  const int32_t gap = evaluated ? (int32_t)boundary_gap(mask) : -1;
  out.flag[i64] = (evaluated && gap >= min_gap) ? (uint8_t)1 : (uint8_t)0;
  if (out.gaps) out.gaps[i64] = gap;
  if (out.masks) out.masks[i64] = mask;
  if (out.counts) out.counts[i64] = (b.met && usable) ? b.count : 0;
}

template <int kSrc>
void boundary_launch(const pcgx_kdtree *t, const TreeView &tv, const XTreeView &xv, const QuerySource &Q, float bound,
                     const float *d_normals, int32_t min_gap, int32_t min_neighbors, const BoundaryOut &out,
                     size_t stack_bytes, hipStream_t st) {
  const dim3 grid(xcd_grid((unsigned)((Q.nq + kBoundaryBlock - 1) / kBoundaryBlock))), block(kBoundaryBlock);
  const GridView g = kSrc == kRangeGrid ? t->grid : GridView{};
  hipLaunchKernelGGL(boundary_kernel<kSrc>, grid, block, stack_bytes, st, g, tv, xv, Q, bound, d_normals, min_gap,
                     min_neighbors, out, xwalk_guard(t->n));
}

// Len() > 0, everything device resident; temporaries from ctx().arena, which the caller has begun
pcgx_status boundary_enqueue(const pcgx_kdtree *t, float radius, const float *d_normals, int32_t min_gap,
                             int32_t min_neighbors, int32_t *d_ids, int32_t *d_n_ids, int32_t *d_gaps, uint64_t *d_masks,
                             int32_t *d_counts, hipStream_t st) {
  const int64_t n = t->n;
  const RangeSrc src = range_source(t);  // as pcgx_kdtree_range_count takes it
  XTreeView xv{};
  if (src == kRangeXWalk) PCGX_TRY(xtree_view(t, &xv, st));
  const TreeView tv = t->view();
  QuerySource Q;
  PCGX_TRY(query_source(t, src, nullptr, n, &Q, st));
  const int ntiles = (int)((n + kRunTile - 1) / kRunTile);
  BoundaryOut out{nullptr, d_gaps, d_masks, d_counts};
  uint32_t *tile_count = nullptr;
  PCGX_TRY(ctx().arena.alloc_n((size_t)n, &out.flag));
  PCGX_TRY(ctx().arena.alloc_n((size_t)ntiles, &tile_count));
  const float bound = radius * radius;
  if (src == kRangeXWalk)
    boundary_launch<kRangeXWalk>(t, tv, xv, Q, bound, d_normals, min_gap, min_neighbors, out,
                                 xwalk_stack_bytes(xv, kBoundaryBlock), st);
  else if (src == kRangeGrid)
    boundary_launch<kRangeGrid>(t, tv, xv, Q, bound, d_normals, min_gap, min_neighbors, out, 0, st);
  else
    boundary_launch<kRangeWalk>(t, tv, xv, Q, bound, d_normals, min_gap, min_neighbors, out,
                                walk_stack_bytes(tv, kBoundaryBlock), st);
  return flags_to_ids_enqueue(out.flag, n, tile_count, d_ids, d_n_ids, st);
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kBoundaryMaxPoints = 0x7fffffff;  // ids are int32 on the device

pcgx_status boundary_check(const char *fn, const pcgx_kdtree *t, float radius, const void *normals, int32_t min_gap,
                           const void *ids, const void *n_ids) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!(radius > 0.0f && radius < __builtin_inff())) return fail(PCGX_E_INVALID, "%s: radius must be finite and > 0", fn);
  if (min_gap < 1 || min_gap > kBoundarySectors) return fail(PCGX_E_INVALID, "%s: min_gap must be 1..64 sectors", fn);
  if (t->n > kBoundaryMaxPoints) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points", fn);
  if (t->n > 0 && (!normals || !ids || !n_ids)) return fail(PCGX_E_INVALID, "%s: NULL normals, ids or n_ids", fn);
  return PCGX_OK;
}

}  // namespace

extern "C" pcgx_status pcgx_kdtree_boundary_dev(const pcgx_kdtree *t, float radius, const float *d_normals,
                                                int32_t min_gap, int32_t min_neighbors, int32_t *d_ids, int32_t *d_n_ids,
                                                int32_t *d_gaps, uint64_t *d_masks, int32_t *d_counts, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(boundary_check("pcgx_kdtree_boundary_dev", t, radius, d_normals, min_gap, d_ids, d_n_ids));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  if (t->n == 0) {
    if (d_n_ids) PCGX_HIP_TRY(hipMemsetAsync(d_n_ids, 0, sizeof(int32_t), st));
    return PCGX_OK;
  }
  PCGX_TRY(ctx().arena.begin(st));
  return boundary_enqueue(t, radius, d_normals, min_gap, min_neighbors, d_ids, d_n_ids, d_gaps, d_masks, d_counts, st);
}

extern "C" pcgx_status pcgx_kdtree_boundary(const pcgx_kdtree *t, float radius, const float *normals, int32_t min_gap,
                                            int32_t min_neighbors, int64_t *ids, int64_t *n_ids, int32_t *gaps,
                                            uint64_t *masks, int32_t *counts) {
  PCGX_API_CALL();
  PCGX_TRY(boundary_check("pcgx_kdtree_boundary", t, radius, normals, min_gap, ids, n_ids));
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
  float *d_nrm = nullptr;
  int32_t *d_out = nullptr, *d_gaps = nullptr, *d_counts = nullptr;  // d_out: ids [n], the count
  uint64_t *d_masks = nullptr;
  PCGX_TRY(ha.alloc_n((size_t)n * 3, &d_nrm));
  PCGX_TRY(staged_upload(d_nrm, normals, (size_t)n * 12, st));
  PCGX_TRY(ha.alloc_n((size_t)n + 1, &d_out));
  if (gaps) PCGX_TRY(ha.alloc_n((size_t)n, &d_gaps));
  if (masks) PCGX_TRY(ha.alloc_n((size_t)n, &d_masks));
  if (counts) PCGX_TRY(ha.alloc_n((size_t)n, &d_counts));
  PCGX_TRY(pcgx_kdtree_boundary_dev(t, radius, d_nrm, min_gap, min_neighbors, d_out, d_out + n, d_gaps, d_masks, d_counts,
                                    st));
  if (gaps) PCGX_TRY(staged_download(gaps, d_gaps, (size_t)n * 4, st));
  if (masks) PCGX_TRY(staged_download(masks, d_masks, (size_t)n * 8, st));
  if (counts) PCGX_TRY(staged_download(counts, d_counts, (size_t)n * 4, st));
  RawVector<int32_t> h((size_t)n + 1);
  PCGX_TRY(staged_download(h.data(), d_out, ((size_t)n + 1) * 4, st));
  for (int64_t i = 0; i < n; i++) ids[i] = h[(size_t)i];
  *n_ids = h[(size_t)n];
  return PCGX_OK;
}
