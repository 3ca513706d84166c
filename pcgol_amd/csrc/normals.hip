// normals.hip -- surface normals from KD-tree radius neighbourhoods (extension: no reference parity).
//
// pcgol has no normal estimation; this is the input the point-to-plane extension (icp.hip, kPlane) needs for a cloud
// that is not synthetic.  For a query q (float32), radius r, viewpoint v (include/pcgx.h, pcgx_kdtree_normals):
//   N(q)   = every point p of the tree with DistSq(p, q) < r*r -- the reference's float32 expression, exactly the set
//            pcgx_kdtree_range_count counts (range.hip) on every kind of handle;
//   count  = |N(q)|; below max(min_neighbors, 3), or when all of N(q) coincide: normal 0, curvature NaN;
//   else, in float64 with d = p - q (centred on the query: small cancellation), mean = sum d / count,
//          C = sum d d^T / count - mean mean^T, eigenvalues l0 <= l1 <= l2:
//          normal = unit eigenvector of l0 turned towards v, curvature = max(l0, 0) / (l0 + l1 + l2);
//          when the float64 trace of C rounds to <= 0 (the neighbours' spread below ~1e-8 of their distance from
//          the query: the moments cancel) nothing can be solved: normal 0, curvature NaN, as if degenerate.
// Nothing is materialised: each lane enumerates its query's neighbours exactly as the range kernels do and keeps
// count, sum d (3), the upper triangle of sum d d^T (6) and the box of the neighbours (6 floats: "all coincide" is
// exact, whatever the summation rounds) in registers, then solves the 3 x 3 eigenproblem in the same kernel by
// cyclic Jacobi in double.  The enumeration is radius_visit (radius_visit.h) over the source pcgx_kdtree_range_count
// takes on that handle (range_source, range_enum.h): the grid, the implicit tree's walk, the patched tree's walk.
// Queries: the caller's, or the tree's own points (q == NULL), as query_source (range_enum.h) lays them out.
// ISS keypoints (keypoints.hip, pcgx_kdtree_iss_keypoints) take their eigenvalues from this kernel: the same moments and
// the same solve, the eigenvalues scaled back by the trace and rounded to float32, and the saliency decided on them
// (keypoint_terms.h) -- two more nullable outputs of normals_finish, the normal itself nullable for that caller.
#include <math.h>
#include <stdlib.h>

#include "cov3.h"
#include "keypoint_terms.h"
#include "radius_visit.h"

namespace pcgx {

constexpr int kNormBlock = kRangeWalkBlock;     // one wave per workgroup: the walks' LDS frame stacks are [level][64]

struct NormOut {
  float *normals;    // [3 nq] or nullptr (ISS)
  float *curvature;  // [nq] or nullptr
  int32_t *counts;   // [nq] or nullptr
  float vx, vy, vz;  // viewpoint
  int32_t min_nb;    // >= 3
  // ISS (nullptr for pcgx_kdtree_normals): l0 <= l1 <= l2 of C, unscaled, l0 clamped at 0, float32; (0, 0, 0) where
  // the normal would be 0.  saliency: iss_saliency of them under the two thresholds.
  float *eigenvalues;  // [3 nq] or nullptr
  float *saliency;     // [nq] or nullptr
  float gamma_21, gamma_32;
};

// count, moments -> normal, curvature of query i (the contract in the file's head)
__device__ __forceinline__ void normals_finish(const NormAcc &a, const float qx, const float qy, const float qz,
                                               const NormOut &O, const int64_t i) {
  float nx = 0.0f, ny = 0.0f, nz = 0.0f, cv = __builtin_nanf("");
  float l0f = 0.0f, l1f = 0.0f, l2f = 0.0f;
  const bool spread = !(a.lox == a.hix && a.loy == a.hiy && a.loz == a.hiz);
  if (a.n >= O.min_nb && spread) {
    double A[3][3], V[3][3];
    norm_acc_cov(a, A);
    const double tr = A[0][0] + A[1][1] + A[2][2];
    if (tr > 0.0) {
      double e0, e1, e2, ux, uy, uz;
      const double l0 = norm_acc_solve(A, V, tr, e0, e1, e2, ux, uy, uz);
      face_viewpoint(ux, uy, uz, O.vx, O.vy, O.vz, qx, qy, qz);
      nx = (float)ux;
      ny = (float)uy;
      nz = (float)uz;
      cv = (float)(fmax(l0, 0.0) / (e0 + e1 + e2));
      if (O.eigenvalues || O.saliency) {  // (the solve works at unit trace: back by the trace)
        const double lo = fmin(e0, e1), hi = fmax(e0, e1);
        l0f = (float)(fmax(l0, 0.0) * tr);
        l1f = (float)(fmax(lo, fmin(hi, e2)) * tr);
        l2f = (float)(fmax(hi, e2) * tr);
      }
    }
  }
  if (O.normals) {
    O.normals[3 * i] = nx;
    O.normals[3 * i + 1] = ny;
    O.normals[3 * i + 2] = nz;
  }
  if (O.curvature) O.curvature[i] = cv;
  if (O.counts) O.counts[i] = a.n;
  if (O.eigenvalues) {
    O.eigenvalues[3 * i] = l0f;
    O.eigenvalues[3 * i + 1] = l1f;
    O.eigenvalues[3 * i + 2] = l2f;
  }
  if (O.saliency) O.saliency[i] = iss_saliency(l0f, l1f, l2f, O.gamma_21, O.gamma_32);
}

template <int kSrc>
__global__ __launch_bounds__(kNormBlock) void normals_kernel(GridView g, TreeView tv, XTreeView xv, QuerySource Q,
                                                             float bound, NormOut O, int64_t guard) {
  extern __shared__ uint32_t s_stack[];
  const uint32_t n_tiles = (uint32_t)((Q.nq + kNormBlock - 1) / kNormBlock);
  const int64_t pos = (int64_t)xcd_tile(blockIdx.x, n_tiles) * kNormBlock + threadIdx.x;
  const bool live = pos < Q.nq;
  int64_t i = 0;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (live) read_query(Q, pos, i, qx, qy, qz);
  const int lane = (int)(threadIdx.x & 63u);
  NormAcc acc;
  acc.clear();
  radius_visit<kSrc>(
      RadiusViews{g, tv, xv, guard}, s_stack + threadIdx.x, kNormBlock, qx, qy, qz, bound, live,
      [&](const float4 &p, float) { acc.add(p.x, p.y, p.z, qx, qy, qz); },
      [&](int owner, float ox, float oy, float oz, auto rows) {  // the partial moments, summed over the wave
        NormAcc part;
        part.clear();
        rows([&](const float4 &p, float) { part.add(p.x, p.y, p.z, ox, oy, oz); });
        part.wave_sum();
        if (lane == owner) acc.merge(part);
      });
  if (!live) return;
  normals_finish(acc, qx, qy, qz, O, i);
}

}  // namespace pcgx

using namespace pcgx;

namespace {

pcgx_status normals_check(const char *fn, const pcgx_kdtree *t, const float *q, int64_t nq, float radius,
                          const float *normals) {
  if (!t || nq < 0) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!(radius > 0.0f) || !(radius < __builtin_inff())) return fail(PCGX_E_INVALID, "%s: radius must be finite and > 0", fn);
  PCGX_TRY(own_query_check(fn, t, q, nq));
  if (nq > 0 && !normals) return fail(PCGX_E_INVALID, "%s: NULL normals", fn);
  return PCGX_OK;
}

}  // namespace

namespace pcgx {

// everything device resident; temporaries from ctx().arena, which the caller has begun
pcgx_status normals_enqueue(const pcgx_kdtree *t, const float *d_q, int64_t nq, float radius, NormOut O, hipStream_t st) {
  const RangeSrc src = range_source(t);  // as pcgx_kdtree_range_count takes it
  XTreeView xv{};
  if (src == kRangeXWalk) PCGX_TRY(xtree_view(t, &xv, st));
  const TreeView tv = t->view();
  QuerySource Q;
  PCGX_TRY(query_source(t, src, d_q, nq, &Q, st));
  if (O.min_nb < 3) O.min_nb = 3;
  const float bound = radius * radius;
  const dim3 grid(xcd_grid((unsigned)((nq + kNormBlock - 1) / kNormBlock))), block(kNormBlock);
  const int64_t guard = xwalk_guard(t->n);
  if (src == kRangeXWalk) {
    hipLaunchKernelGGL(normals_kernel<kRangeXWalk>, grid, block, xwalk_stack_bytes(xv, kNormBlock), st, GridView{}, tv, xv,
                       Q, bound, O, guard);
  } else if (src == kRangeGrid) {
    hipLaunchKernelGGL(normals_kernel<kRangeGrid>, grid, block, 0, st, t->grid, tv, xv, Q, bound, O, guard);
  } else {
    hipLaunchKernelGGL(normals_kernel<kRangeWalk>, grid, block, walk_stack_bytes(tv, kNormBlock), st, GridView{}, tv, xv, Q,
                       bound, O, guard);
  }
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

// The eigenvalue stage of ISS keypoints (keypoints.hip): the tree's own points, eigenvalues [3 Len()] (may be nullptr)
// and saliency [Len()] in id order.  The caller has begun ctx().arena.
pcgx_status normals_iss_enqueue(const pcgx_kdtree *t, float radius, int32_t min_neighbors, float gamma_21, float gamma_32,
                                float *d_eigenvalues, float *d_saliency, hipStream_t st) {
  NormOut O{};
  O.min_nb = min_neighbors;
  O.eigenvalues = d_eigenvalues;
  O.saliency = d_saliency;
  O.gamma_21 = gamma_21;
  O.gamma_32 = gamma_32;
  return normals_enqueue(t, nullptr, t->n, radius, O, st);
}

}  // namespace pcgx

extern "C" pcgx_status pcgx_kdtree_normals_dev(const pcgx_kdtree *t, const float *d_q, int64_t nq, float radius,
                                               const float viewpoint[3], int32_t min_neighbors, float *d_normals,
                                               float *d_curvature, int32_t *d_counts, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(normals_check("pcgx_kdtree_normals_dev", t, d_q, nq, radius, d_normals));
  if (nq == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  PCGX_TRY(ctx().arena.begin(st));
  NormOut O{};
  O.normals = d_normals;
  O.curvature = d_curvature;
  O.counts = d_counts;
  O.min_nb = min_neighbors;
  if (viewpoint) {
    O.vx = viewpoint[0];
    O.vy = viewpoint[1];
    O.vz = viewpoint[2];
  }
  return normals_enqueue(t, d_q, nq, radius, O, st);
}

extern "C" pcgx_status pcgx_kdtree_normals(const pcgx_kdtree *t, const float *q, int64_t nq, float radius,
                                           const float viewpoint[3], int32_t min_neighbors, float *normals,
                                           float *curvature, int32_t *counts) {
  PCGX_API_CALL();
  PCGX_TRY(normals_check("pcgx_kdtree_normals", t, q, nq, radius, normals));
  if (nq == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  // always on the device, a single query too: the moments and the solve are the kernel's, not a host restatement
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_q = nullptr, *d_n = nullptr, *d_c = nullptr;
  int32_t *d_k = nullptr;
  if (q) {
    PCGX_TRY(ha.alloc_n((size_t)nq * 3, &d_q));
    PCGX_TRY(staged_upload(d_q, q, (size_t)nq * 12, st));
  }
  PCGX_TRY(ha.alloc_n((size_t)nq * 3, &d_n));
  if (curvature) PCGX_TRY(ha.alloc_n((size_t)nq, &d_c));
  if (counts) PCGX_TRY(ha.alloc_n((size_t)nq, &d_k));
  PCGX_TRY(pcgx_kdtree_normals_dev(t, d_q, nq, radius, viewpoint, min_neighbors, d_n, d_c, d_k, st));
  PCGX_TRY(staged_download(normals, d_n, (size_t)nq * 12, st));
  if (curvature) PCGX_TRY(staged_download(curvature, d_c, (size_t)nq * 4, st));
  if (counts) PCGX_TRY(staged_download(counts, d_k, (size_t)nq * 4, st));
  return PCGX_OK;
}
