// mls.hip -- moving-least-squares smoothing over KD-tree radius neighbourhoods (extension: no reference parity).
//
// pcgol cannot put noisy points back onto their surface; every stage of the coarse-to-fine chain (normals, keypoints,
// FPFH, the point-to-plane and GICP Fits) assumes they lie on it.  For a query q (float32), radius r, sigma, order
// (include/pcgx.h, pcgx_kdtree_mls; the arithmetic is mls_terms.h):
//   N(q)  = every point p of the tree with DistSq(p, q) < r*r, exactly the set pcgx_kdtree_range_count counts;
//   pass 1: the moments of N(q) and the 3 x 3 eigen-solve, as normals.hip has them -> the reference plane through the
//           centroid, its axes u, v, and the query's projection q + d0 onto it (kind 1; kind 0 where normals answer
//           "degenerate": the query comes back unchanged);
//   pass 2 (order 2, count >= 6): N(q) is enumerated again for the 28 float64 sums of the Gauss-weighted normal
//           equations of a quadratic height field over the plane; a 6 x 6 Cholesky in registers, and the query moves
//           to the field's height at its own place (kind 2), with the field's normal.
// Nothing is materialised; one query per lane, each pass one radius_visit (radius_visit.h) as normals_kernel's.  A fat
// row is the whole wave's work in pass 2 as in pass 1: the other 63 lanes fetch the owner's frame, add their share of
// the row, and the partial sums are summed over the wave.  A lane without a polynomial to fit (no query, kind 0, order
// 1's kind 1, fewer than 6 neighbours) is not live in pass 2.  The order of every sum is fixed by the handle and the
// launch: the same call gives the same bits.
#include <math.h>
#include <stdlib.h>

#include "mls_terms.h"
#include "radius_visit.h"

namespace pcgx {

constexpr int kMlsBlock = kRangeWalkBlock;  // one wave per workgroup: the walks' LDS frame stacks are [level][64]

struct MlsOut {
  float *points;     // [3 nq]
  float *normals;    // [3 nq] or nullptr
  int32_t *kinds;    // [nq] or nullptr
  int32_t *counts;   // [nq] or nullptr
  float vx, vy, vz;  // viewpoint
  int32_t min_nb;    // >= 3
  float radius, sigma;
};

// the owner lane's frame into every lane (all 64 lanes must be here)
__device__ __forceinline__ MlsFrame mls_frame_of(const MlsFrame &F, const int owner) {
  MlsFrame G;
  G.nx = __shfl(F.nx, owner); G.ny = __shfl(F.ny, owner); G.nz = __shfl(F.nz, owner);
  G.ux = __shfl(F.ux, owner); G.uy = __shfl(F.uy, owner); G.uz = __shfl(F.uz, owner);
  G.vx = __shfl(F.vx, owner); G.vy = __shfl(F.vy, owner); G.vz = __shfl(F.vz, owner);
  G.d0x = __shfl(F.d0x, owner); G.d0y = __shfl(F.d0y, owner); G.d0z = __shfl(F.d0z, owner);
  G.inv_r = __shfl(F.inv_r, owner); G.inv_s2 = __shfl(F.inv_s2, owner);
  return G;
}

template <int kSrc, int kOrder>
__global__ __launch_bounds__(kMlsBlock) void mls_kernel(GridView g, TreeView tv, XTreeView xv, QuerySource Q, float bound,
                                                        MlsOut O, int64_t guard) {
  extern __shared__ uint32_t s_stack[];
  const uint32_t n_tiles = (uint32_t)((Q.nq + kMlsBlock - 1) / kMlsBlock);
  const int64_t pos = (int64_t)xcd_tile(blockIdx.x, n_tiles) * kMlsBlock + threadIdx.x;
  const bool live = pos < Q.nq;
  int64_t i = 0;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (live) read_query(Q, pos, i, qx, qy, qz);
  const int lane = (int)(threadIdx.x & 63u);
  const RadiusViews V{g, tv, xv, guard};

  // pass 1: the moments, as normals_kernel sums them
  NormAcc acc;
  acc.clear();
  radius_visit<kSrc>(
      V, s_stack + threadIdx.x, kMlsBlock, qx, qy, qz, bound, live,
      [&](const float4 &p, float) { acc.add(p.x, p.y, p.z, qx, qy, qz); },
      [&](int owner, float ox, float oy, float oz, auto rows) {
        NormAcc part;
        part.clear();
        rows([&](const float4 &p, float) { part.add(p.x, p.y, p.z, ox, oy, oz); });
        part.wave_sum();
        if (lane == owner) acc.merge(part);
      });
  MlsFrame F{};
  const bool framed = live && mls_frame(acc, O.min_nb, O.radius, O.sigma, F);

  // pass 2: the normal equations of the lanes that fit a polynomial (the others have nothing to enumerate)
  MlsAcc eq;
  eq.clear();
  const bool poly = kOrder == 2 && framed && acc.n >= kMlsBasis;
  if constexpr (kOrder == 2) {
    radius_visit<kSrc>(
        V, s_stack + threadIdx.x, kMlsBlock, qx, qy, qz, bound, poly,
        [&](const float4 &p, float) { eq.add(p.x, p.y, p.z, qx, qy, qz, F); },
        [&](int owner, float ox, float oy, float oz, auto rows) {
          const MlsFrame G = mls_frame_of(F, owner);
          MlsAcc part;
          part.clear();
          rows([&](const float4 &p, float) { part.add(p.x, p.y, p.z, ox, oy, oz, G); });
          part.wave_sum();
          if (lane == owner) eq.merge(part);
        });
  }
  if (!live) return;
  const MlsResult R = mls_finish(framed, F, poly, eq, O.radius, qx, qy, qz, O.vx, O.vy, O.vz);
  O.points[3 * i] = R.px;
  O.points[3 * i + 1] = R.py;
  O.points[3 * i + 2] = R.pz;
  if (O.normals) {
    O.normals[3 * i] = R.nx;
    O.normals[3 * i + 1] = R.ny;
    O.normals[3 * i + 2] = R.nz;
  }
  if (O.kinds) O.kinds[i] = R.kind;
  if (O.counts) O.counts[i] = acc.n;
}

}  // namespace pcgx

using namespace pcgx;

namespace {

pcgx_status mls_check(const char *fn, const pcgx_kdtree *t, const float *q, int64_t nq, float radius, float sigma,
                      int32_t order, const float *points) {
  if (!t || nq < 0) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!(radius > 0.0f) || !(radius < __builtin_inff())) return fail(PCGX_E_INVALID, "%s: radius must be finite and > 0", fn);
  if (!(sigma > 0.0f) || !(sigma < __builtin_inff())) return fail(PCGX_E_INVALID, "%s: sigma must be finite and > 0", fn);
  if (order != 1 && order != 2) return fail(PCGX_E_INVALID, "%s: order must be 1 or 2", fn);
  PCGX_TRY(own_query_check(fn, t, q, nq));
  if (nq > 0 && !points) return fail(PCGX_E_INVALID, "%s: NULL points", fn);
  return PCGX_OK;
}

template <int kOrder>
void mls_launch(const pcgx_kdtree *t, const RangeSrc src, const TreeView &tv, const XTreeView &xv, const QuerySource &Q,
                const float bound, const MlsOut &O, hipStream_t st) {
  const dim3 grid(xcd_grid((unsigned)((Q.nq + kMlsBlock - 1) / kMlsBlock))), block(kMlsBlock);
  const int64_t guard = xwalk_guard(t->n);
  if (src == kRangeXWalk) {
    hipLaunchKernelGGL((mls_kernel<kRangeXWalk, kOrder>), grid, block, xwalk_stack_bytes(xv, kMlsBlock), st, GridView{}, tv,
                       xv, Q, bound, O, guard);
  } else if (src == kRangeGrid) {
    hipLaunchKernelGGL((mls_kernel<kRangeGrid, kOrder>), grid, block, 0, st, t->grid, tv, xv, Q, bound, O, guard);
  } else {
    hipLaunchKernelGGL((mls_kernel<kRangeWalk, kOrder>), grid, block, walk_stack_bytes(tv, kMlsBlock), st, GridView{}, tv,
                       xv, Q, bound, O, guard);
  }
}

// everything device resident; temporaries from ctx().arena, which the caller has begun
pcgx_status mls_enqueue(const pcgx_kdtree *t, const float *d_q, int64_t nq, int32_t order, MlsOut O, hipStream_t st) {
  const RangeSrc src = range_source(t);  // as pcgx_kdtree_range_count takes it
  XTreeView xv{};
  if (src == kRangeXWalk) PCGX_TRY(xtree_view(t, &xv, st));
  const TreeView tv = t->view();
  QuerySource Q;
  PCGX_TRY(query_source(t, src, d_q, nq, &Q, st));
  if (O.min_nb < 3) O.min_nb = 3;
  const float bound = O.radius * O.radius;
  if (order == 2) mls_launch<2>(t, src, tv, xv, Q, bound, O, st);
  else mls_launch<1>(t, src, tv, xv, Q, bound, O, st);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

}  // namespace

extern "C" pcgx_status pcgx_kdtree_mls_dev(const pcgx_kdtree *t, const float *d_q, int64_t nq, float radius, float sigma,
                                           int32_t order, int32_t min_neighbors, const float viewpoint[3], float *d_points,
                                           float *d_normals, int32_t *d_kinds, int32_t *d_counts, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(mls_check("pcgx_kdtree_mls_dev", t, d_q, nq, radius, sigma, order, d_points));
  if (nq == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  PCGX_TRY(ctx().arena.begin(st));
  MlsOut O{};
  O.points = d_points;
  O.normals = d_normals;
  O.kinds = d_kinds;
  O.counts = d_counts;
  O.min_nb = min_neighbors;
  O.radius = radius;
  O.sigma = sigma;
  if (viewpoint) {
    O.vx = viewpoint[0];
    O.vy = viewpoint[1];
    O.vz = viewpoint[2];
  }
  return mls_enqueue(t, d_q, nq, order, O, st);
}

extern "C" pcgx_status pcgx_kdtree_mls(const pcgx_kdtree *t, const float *q, int64_t nq, float radius, float sigma,
                                       int32_t order, int32_t min_neighbors, const float viewpoint[3], float *points,
                                       float *normals, int32_t *kinds, int32_t *counts) {
  PCGX_API_CALL();
  PCGX_TRY(mls_check("pcgx_kdtree_mls", t, q, nq, radius, sigma, order, points));
  if (nq == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  // always on the device, a single query too: the sums and the solves are the kernel's, not a host restatement
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_q = nullptr, *d_p = nullptr, *d_n = nullptr;
  int32_t *d_kind = nullptr, *d_k = nullptr;
  if (q) {
    PCGX_TRY(ha.alloc_n((size_t)nq * 3, &d_q));
    PCGX_TRY(staged_upload(d_q, q, (size_t)nq * 12, st));
  }
  PCGX_TRY(ha.alloc_n((size_t)nq * 3, &d_p));
  if (normals) PCGX_TRY(ha.alloc_n((size_t)nq * 3, &d_n));
  if (kinds) PCGX_TRY(ha.alloc_n((size_t)nq, &d_kind));
  if (counts) PCGX_TRY(ha.alloc_n((size_t)nq, &d_k));
  PCGX_TRY(pcgx_kdtree_mls_dev(t, d_q, nq, radius, sigma, order, min_neighbors, viewpoint, d_p, d_n, d_kind, d_k, st));
  PCGX_TRY(staged_download(points, d_p, (size_t)nq * 12, st));
  if (normals) PCGX_TRY(staged_download(normals, d_n, (size_t)nq * 12, st));
  if (kinds) PCGX_TRY(staged_download(kinds, d_kind, (size_t)nq * 4, st));
  if (counts) PCGX_TRY(staged_download(counts, d_k, (size_t)nq * 4, st));
  return PCGX_OK;
}
