// knearest.hip -- k nearest neighbours on a KD-tree handle (extension: no reference counterpart).
//
// pcgol answers Nearest (k = 1) and Range (a fixed radius); this is the k closest points, the query statistical outlier
// removal (sor.hip) is built on.  For query q, 1 <= k <= 64, bound B = max_range^2 (include/pcgx.h, pcgx_kdtree_knearest):
//   the k points p of the tree with the smallest (DistSq(p, q), id), lexicographic, among those with DistSq < B
//   (Range's rule; DistSq is the reference's float32 expression ref_dist_sq), ascending.
// Ties go by id, not by visit order: the answer is a function of the cloud alone, so no source ever has to fall back to
// another because of a tie, and a brute-force oracle checks it.  Each lane keeps its query's best k as 64-bit keys
// {bits(DistSq) << 32 | id} -- DistSq >= 0, so the bits order as the floats do and one integer compare is the
// lexicographic one -- sorted ascending in LDS laid out [slot][lane] (a runtime-indexed register array would go to
// scratch), inserted by a short insertion sort.  d_k is the k-th DistSq once k are held.  Three sources, as
// pcgx_kdtree_range_count takes them (range_source, range_enum.h):
//   grid  (kRangeGrid): the 3 x 3 x 3 cells around the query, then shells; accepted when grid_cover(min(d_k, B)) lies
//         inside the box scanned (the certificate knn_grid.h uses for k = 1).  A box beyond kGridWide cells of the
//         query's own cell goes to the implicit-tree walk below, in the same lane.  The shells' rows are scanned as
//         Range's are (RowScan, range_enum.h): rows of kRangeFatRow records and more (a site of the cloud taken
//         thousands of times) by the whole wave, the owner inserting what beats its k-th key.
//   walk  (kRangeWalk: no grid, PCGX_RANGE_WALK=1): range_walk_nodes over the implicit tree, hits on B, a side pruned
//         when fromPivotSq > min(d_k, B) (strict: an equal-DistSq point with a smaller id may lie beyond the plane),
//         re-tested when a frame is popped;
//   xwalk (kRangeXWalk: a handle that has seen DeletePoint): the patched tree's walk (knn_xwalk.h), same pruning.
// Non-finite queries find nothing (no DistSq of theirs compares below B).  Queries: the caller's, or the tree's own
// points (q == NULL), as query_source (range_enum.h) lays them out.  SOR mode writes no ids: only the mean of
// sqrt(DistSq) over the first mean_k entries other than the query's own id, in float64 (sor.hip).  Covariance mode
// (kCov, pcgx_kdtree_covariances) writes no ids either: after the search the lane fetches each listed point's xyz by id
// (the id -> node map range_inverse_map makes, or the patched tree's copy by id), sums NormAcc (cov3.h) in the list's
// (DistSq, id) order -- so the result is a function of the query and the cloud alone -- and solves as normals.hip does.
#include <math.h>
#include <stdlib.h>

#include <type_traits>

#include "cov3.h"
#include "knn_grid.h"
#include "knn_xwalk.h"
#include "range_walk.h"

namespace pcgx {

constexpr int kKnnKBlock = kRangeWalkBlock;  // one wave per workgroup: the top-k lists and walk stacks are [.][64] in LDS
constexpr int kKnnMaxK = 64;

struct KnnOut {
  int32_t *ids;      // [nq * k] (not SOR)
  float *dsq;        // [nq * k] (not SOR)
  int32_t *counts;   // [nq] or nullptr
  double *mean;      // SOR: [nq] by id, compact
  int32_t mean_k;    // SOR: k - 1
};

// Covariance mode: the outputs, and where a listed neighbour's xyz is fetched by id
struct CovOut {
  float *cov6;          // [6 nq]: xx, xy, xz, yy, yz, zz
  float *normals;       // [3 nq] or nullptr
  int32_t *counts;      // [nq] or nullptr
  const uint32_t *inv;  // grid, walk: id -> BFS slot of its node in the implicit tree (range_inverse_map)
  const float *xyz;     // patched tree: the cloud's points by id (t->d_xsrc)
  float vx, vy, vz;     // viewpoint of the normals
  float eps;            // PLANE: I - (1 - eps) u u^T
  int32_t plane;        // PCGX_COV_PLANE, else PCGX_COV_RAW
};

// moments of the list -> covariance and normal of query i (include/pcgx.h, pcgx_kdtree_covariances)
__device__ __forceinline__ void covariance_finish(const NormAcc &a, const float qx, const float qy, const float qz,
                                                  const CovOut &O, const int64_t i) {
  // degenerate (fewer than 3, or all at one place): I for PLANE, 0 for RAW, normal 0
  const double diag = O.plane ? 1.0 : 0.0;
  double cxx = diag, cxy = 0.0, cxz = 0.0, cyy = diag, cyz = 0.0, czz = diag;
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (a.n >= 3 && !(a.lox == a.hix && a.loy == a.hiy && a.loz == a.hiz)) {
    double A[3][3], V[3][3];
    norm_acc_cov(a, A);
    if (!O.plane) {
      cxx = A[0][0]; cxy = A[0][1]; cxz = A[0][2]; cyy = A[1][1]; cyz = A[1][2]; czz = A[2][2];
    }
    // (tr > 0 for a spread neighbourhood unless rounding cancels it: then PLANE and the normal as if degenerate)
    const double tr = A[0][0] + A[1][1] + A[2][2];
    if ((O.plane || O.normals) && tr > 0.0) {
      double e0, e1, e2, ux, uy, uz;
      norm_acc_solve(A, V, tr, e0, e1, e2, ux, uy, uz);
      if (O.plane) {  // V diag(eps, 1, 1) V^T
        const double f = 1.0 - (double)O.eps;
        cxx = 1.0 - f * ux * ux; cxy = -f * ux * uy; cxz = -f * ux * uz;
        cyy = 1.0 - f * uy * uy; cyz = -f * uy * uz; czz = 1.0 - f * uz * uz;
      }
      face_viewpoint(ux, uy, uz, O.vx, O.vy, O.vz, qx, qy, qz);
      nx = (float)ux;
      ny = (float)uy;
      nz = (float)uz;
    }
  }
  float *c = O.cov6 + 6 * i;
  c[0] = (float)cxx; c[1] = (float)cxy; c[2] = (float)cxz; c[3] = (float)cyy; c[4] = (float)cyz; c[5] = (float)czz;
  if (O.normals) {
    O.normals[3 * i] = nx;
    O.normals[3 * i + 1] = ny;
    O.normals[3 * i + 2] = nz;
  }
}

// One lane's best k, ascending, in LDS column `col` (slot s at col[s * 64]).
struct TopK {
  uint64_t *col;
  int k, c;        // capacity, held
  uint64_t worst;  // the k-th key once k are held, else all ones
  float mr2;       // max_range^2
  float lim;       // min(d_k, mr2): a point must have DistSq below it (equal: only with a smaller id)

  __device__ __forceinline__ void init(uint64_t *column, int kk, float b) {
    col = column;
    k = kk;
    c = 0;
    worst = ~0ull;
    mr2 = b;
    lim = b;
  }
  __device__ __forceinline__ static uint64_t key_of(float d, uint32_t id) {
    return ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)id;
  }
  // the key of a point that may go in (Range's rule d < max_range^2 first), or all ones
  __device__ __forceinline__ uint64_t candidate(float d, uint32_t id) const {
    if (!(d < mr2)) return ~0ull;
    const uint64_t key = key_of(d, id);
    return key < worst ? key : ~0ull;
  }
  __device__ __forceinline__ void insert_key(uint64_t key) {
    if (key >= worst) return;
    int j = c < k ? c : k - 1;
    while (j > 0) {
      const uint64_t prev = col[(j - 1) * kKnnKBlock];
      if (prev <= key) break;
      col[j * kKnnKBlock] = prev;
      j--;
    }
    col[j * kKnnKBlock] = key;
    if (c < k) c++;
    if (c == k) {
      worst = col[(k - 1) * kKnnKBlock];
      lim = __uint_as_float((uint32_t)(worst >> 32));
    }
  }
  __device__ __forceinline__ void take(float d, uint32_t id) {
    const uint64_t key = candidate(d, id);
    if (key != ~0ull) insert_key(key);
  }
  __device__ __forceinline__ void take(const float4 &p, float qx, float qy, float qz) {
    take(ref_dist_sq(p.x, p.y, p.z, qx, qy, qz), __float_as_uint(p.w));
  }
  __device__ __forceinline__ void clear() {
    c = 0;
    worst = ~0ull;
    lim = mr2;
  }
};

// (kCov: the covariance mode's outputs take KnnOut's place, so the other modes' arguments and code stay as they were)
template <int kSrc, bool kSor, bool kCov = false>
__global__ __launch_bounds__(kKnnKBlock) void knearest_kernel(GridView g, TreeView tv, XTreeView xv, QuerySource Q, int32_t k,
                                                              float mr2, std::conditional_t<kCov, CovOut, KnnOut> O,
                                                              int64_t guard) {
  extern __shared__ uint64_t s_knn[];  // [k][64] keys, then the walk's frames [levels][64]
  uint32_t *s_stack = reinterpret_cast<uint32_t *>(s_knn + (size_t)k * kKnnKBlock);
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t n_tiles = (uint32_t)((Q.nq + kKnnKBlock - 1) / kKnnKBlock);
  const int64_t pos = (int64_t)xcd_tile(blockIdx.x, n_tiles) * kKnnKBlock + threadIdx.x;
  // (the grid path keeps every lane of the wave to the end: fat rows are scanned by all 64)
  const bool live = pos < Q.nq;
  if (kSrc != kRangeGrid && !live) return;
  int64_t i = 0;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (live) read_query(Q, pos, i, qx, qy, qz);
  const bool finite = isfinite(qx) && isfinite(qy) && isfinite(qz);  // else: nothing (no DistSq compares below B)
  TopK top;
  top.init(s_knn + lane, k, mr2);
  // the implicit tree: hits on max_range^2 (TopK applies the key test), pruned on the shrinking min(d_k, B)
  auto walk_tree = [&]() {
    range_walk_nodes<true>(tv, s_stack + threadIdx.x, kKnnKBlock, qx, qy, qz, mr2, [&]() { return top.lim; },
                           [&](const float4 &nd, float d) { top.take(d, __float_as_uint(nd.w)); });
  };
  if constexpr (kSrc == kRangeGrid) {
    bool active = live && finite, walk = false;
    GridBox box;  // scanned so far; empty at first (z1 < z0)
    box.x0 = box.y0 = box.z0 = 1;
    box.x1 = box.y1 = box.z1 = 0;
    const int cx = grid_cell(qx, g.lo[0], g.inv_h, g.nx), cy = grid_cell(qy, g.lo[1], g.inv_h, g.ny),
              cz = grid_cell(qz, g.lo[2], g.inv_h, g.nz);
    GridBox nb;  // the box after this round's shell
    nb.x0 = max(cx - 1, 0); nb.x1 = min(cx + 1, g.nx - 1);
    nb.y0 = max(cy - 1, 0); nb.y1 = min(cy + 1, g.ny - 1);
    nb.z0 = max(cz - 1, 0); nb.z1 = min(cz + 1, g.nz - 1);
    // (one record at a time: four in flight take 68 VGPRs, occupancy 7 instead of 8)
    auto take = [&](const float4 &p) { top.take(p, qx, qy, qz); };
    // the owner of a fat row inserts what beats its k-th key, 64 records at a time
    auto fat = [&](int owner, uint32_t rf, uint32_t re, float ox, float oy, float oz) {
      for (uint32_t base = rf; base < re; base += 64u) {  // uniform
        const uint32_t ow_lo = (uint32_t)__shfl((int)(uint32_t)top.worst, owner);
        const uint32_t ow_hi = (uint32_t)__shfl((int)(uint32_t)(top.worst >> 32), owner);
        const uint64_t ow = ((uint64_t)ow_hi << 32) | ow_lo;
        uint64_t key = ~0ull;
        const uint32_t r = base + (uint32_t)lane;
        if (r < re) {
          const float4 p = g.pts[r];
          const float d = ref_dist_sq(p.x, p.y, p.z, ox, oy, oz);
          if (d < mr2) {
            const uint64_t kk = TopK::key_of(d, __float_as_uint(p.w));
            key = kk < ow ? kk : ~0ull;
          }
        }
        unsigned long long cand = __ballot(key != ~0ull);
        while (cand != 0ull) {  // uniform; the owner inserts (and drops what its k-th key no longer admits)
          const int l = __builtin_ctzll(cand);
          cand &= cand - 1ull;
          const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)key, l);
          const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(key >> 32), l);
          if (lane == owner) top.insert_key(((uint64_t)hi << 32) | lo);
        }
      }
    };
    // every round: each active lane scans the shell nb \ box (up to two fat rows set aside), the wave scans the fat
    // rows, each lane checks its certificate and picks the next shell, or leaves for the walk
    while (__ballot(active) != 0ull) {
      RowScan rows;
      if (active) {
        for (int z = nb.z0; z <= nb.z1; z++) {
          for (int y = nb.y0; y <= nb.y1; y++) {
            const bool inner = z >= box.z0 && z <= box.z1 && y >= box.y0 && y <= box.y1;
            // a row inside the old box in y and z: only its new ends; else the whole row
            for (int part = 0; part < (inner ? 2 : 1); part++) {
              const int x0 = inner && part == 1 ? box.x1 + 1 : nb.x0;
              const int x1 = inner && part == 0 ? box.x0 - 1 : nb.x1;
              if (x0 <= x1) rows.row<1>(g, grid_row(g, z, y, x0, x1), take);
            }
          }
        }
      }
      rows.share(qx, qy, qz, fat);
      if (active) {
        const GridBox cov = grid_cover(g, qx, qy, qz, top.lim);
        box = nb;
        if (box_inside(cov, box)) {
          active = false;
        } else {
          // grow towards the cover, one cell per side a round while fewer than k are held (the cover is then the
          // whole of max_range), straight to it once d_k is known
          const bool full = top.c == top.k;
          nb.x0 = cov.x0 < box.x0 ? (full ? cov.x0 : max(cov.x0, box.x0 - 1)) : box.x0;
          nb.y0 = cov.y0 < box.y0 ? (full ? cov.y0 : max(cov.y0, box.y0 - 1)) : box.y0;
          nb.z0 = cov.z0 < box.z0 ? (full ? cov.z0 : max(cov.z0, box.z0 - 1)) : box.z0;
          nb.x1 = cov.x1 > box.x1 ? (full ? cov.x1 : min(cov.x1, box.x1 + 1)) : box.x1;
          nb.y1 = cov.y1 > box.y1 ? (full ? cov.y1 : min(cov.y1, box.y1 + 1)) : box.y1;
          nb.z1 = cov.z1 > box.z1 ? (full ? cov.z1 : min(cov.z1, box.z1 + 1)) : box.z1;
          if (nb.x0 < cx - kGridWide || nb.x1 > cx + kGridWide || nb.y0 < cy - kGridWide || nb.y1 > cy + kGridWide ||
              nb.z0 < cz - kGridWide || nb.z1 > cz + kGridWide) {
            active = false;
            walk = true;
          }
        }
      }
    }
    if (!live) return;
    if (walk) {  // the box would leave kGridWide: the implicit tree, from nothing
      top.clear();
      walk_tree();
    }
  } else if constexpr (kSrc == kRangeWalk) {
    if (finite) walk_tree();
  } else {
    if (finite) {
      auto hit = [&](const float4 &nd, float d) {
        top.take(d, __float_as_uint(nd.w));
        return true;
      };
      xwalk(xv, s_stack + threadIdx.x, kKnnKBlock, qx, qy, qz, guard, [&]() { return top.lim; }, hit, hit);
    }
  }
  if constexpr (kCov) {
    // the listed points by id, in the list's (DistSq, id) order
    NormAcc acc;
    acc.clear();
    for (int s = 0; s < top.c; s++) {
      const uint32_t id = (uint32_t)top.col[s * kKnnKBlock];
      float px, py, pz;
      if constexpr (kSrc == kRangeXWalk) {
        px = O.xyz[3 * (size_t)id];
        py = O.xyz[3 * (size_t)id + 1];
        pz = O.xyz[3 * (size_t)id + 2];
      } else {
        const float4 nd = node_at(tv.nodes, O.inv[id]);
        px = nd.x;
        py = nd.y;
        pz = nd.z;
      }
      acc.add(px, py, pz, qx, qy, qz);
    }
    covariance_finish(acc, qx, qy, qz, O, i);
  } else if constexpr (kSor) {
    // the first mean_k entries other than the query's own id, float64 in ascending order
    double sum = 0.0;
    int taken = 0;
    bool self = false;
    for (int s = 0; s < top.c && taken < O.mean_k; s++) {
      const uint64_t key = top.col[s * kKnnKBlock];
      if (!self && (int64_t)(uint32_t)key == i) {
        self = true;
        continue;
      }
      sum += sqrt((double)__uint_as_float((uint32_t)(key >> 32)));
      taken++;
    }
    O.mean[i] = sum / (double)O.mean_k;
  } else {
    const int64_t row = i * (int64_t)k;
    for (int s = 0; s < k; s++) {
      int32_t id = -1;
      float d = mr2;
      if (s < top.c) {
        const uint64_t key = top.col[s * kKnnKBlock];
        id = (int32_t)(uint32_t)key;
        d = __uint_as_float((uint32_t)(key >> 32));
      }
      O.ids[row + s] = id;
      O.dsq[row + s] = d;
    }
  }
  if (O.counts) O.counts[i] = top.c;
}

template <bool kSor, bool kCov = false>
pcgx_status knearest_launch(const pcgx_kdtree *t, const float *d_q, int64_t nq, int32_t k, float max_range,
                            std::conditional_t<kCov, CovOut, KnnOut> O, hipStream_t st) {
  PCGX_TRY(ctx().arena.begin(st));
  const RangeSrc src = range_source(t);  // as pcgx_kdtree_range_count takes it
  XTreeView xv{};
  if (src == kRangeXWalk) PCGX_TRY(xtree_view(t, &xv, st));
  if constexpr (kCov) {  // where the kernel finds a listed point's xyz (xtree_view made d_xsrc)
    if (src == kRangeXWalk) O.xyz = t->d_xsrc;
    else PCGX_TRY(range_inverse_map(t, &O.inv, st));
  }
  const TreeView tv = t->view();
  QuerySource Q;
  PCGX_TRY(query_source(t, src, d_q, nq, &Q, st));
  const float mr2 = max_range * max_range;
  const dim3 grid(xcd_grid((unsigned)((nq + kKnnKBlock - 1) / kKnnKBlock))), block(kKnnKBlock);
  const int64_t guard = xwalk_guard(t->n);
  const size_t list_bytes = (size_t)k * kKnnKBlock * sizeof(uint64_t);
  if (src == kRangeXWalk) {
    const size_t lds = list_bytes + xwalk_stack_bytes(xv, kKnnKBlock);
    hipLaunchKernelGGL((knearest_kernel<kRangeXWalk, kSor, kCov>), grid, block, lds, st, GridView{}, tv, xv, Q, k, mr2, O, guard);
  } else if (src == kRangeGrid) {
    hipLaunchKernelGGL((knearest_kernel<kRangeGrid, kSor, kCov>), grid, block, list_bytes + walk_stack_bytes(tv, kKnnKBlock), st,
                       t->grid, tv, xv, Q, k, mr2, O, guard);
  } else {
    hipLaunchKernelGGL((knearest_kernel<kRangeWalk, kSor, kCov>), grid, block, list_bytes + walk_stack_bytes(tv, kKnnKBlock), st,
                       GridView{}, tv, xv, Q, k, mr2, O, guard);
  }
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

pcgx_status knearest_sor_enqueue(const pcgx_kdtree *t, int32_t mean_k, double *d_mean, hipStream_t st) {
  KnnOut O{nullptr, nullptr, nullptr, d_mean, mean_k};
  return knearest_launch<true>(t, nullptr, t->n, mean_k + 1, __builtin_inff(), O, st);
}

}  // namespace pcgx

using namespace pcgx;

namespace {

pcgx_status knearest_check(const char *fn, const pcgx_kdtree *t, const float *q, int64_t nq, int32_t k, float max_range,
                           const void *ids, const void *dist_sq) {
  if (!t || nq < 0) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (k < 1 || k > kKnnMaxK) return fail(PCGX_E_INVALID, "%s: k = %d outside [1, %d]", fn, (int)k, kKnnMaxK);
  if (!(max_range >= 0.0f)) return fail(PCGX_E_INVALID, "%s: max_range must be >= 0 or +inf", fn);
  PCGX_TRY(own_query_check(fn, t, q, nq));
  if (nq > 0 && (!ids || !dist_sq)) return fail(PCGX_E_INVALID, "%s: NULL ids / dist_sq", fn);
  return PCGX_OK;
}

pcgx_status covariances_check(const char *fn, const pcgx_kdtree *t, const float *q, int64_t nq, int32_t k,
                              float max_range, int32_t mode, float epsilon, const float *cov6) {
  if (!cov6 && nq > 0) return fail(PCGX_E_INVALID, "%s: NULL cov6", fn);
  PCGX_TRY(knearest_check(fn, t, q, nq, k, max_range, cov6, cov6));
  if (mode != PCGX_COV_RAW && mode != PCGX_COV_PLANE) return fail(PCGX_E_INVALID, "%s: unknown mode %d", fn, (int)mode);
  if (!(epsilon > 0.0f && epsilon <= 1.0f)) return fail(PCGX_E_INVALID, "%s: epsilon must lie in (0, 1]", fn);
  return PCGX_OK;
}

}  // namespace

extern "C" pcgx_status pcgx_kdtree_knearest_dev(const pcgx_kdtree *t, const float *d_q, int64_t nq, int32_t k,
                                                float max_range, int32_t *d_ids, float *d_dist_sq, int32_t *d_counts,
                                                void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(knearest_check("pcgx_kdtree_knearest_dev", t, d_q, nq, k, max_range, d_ids, d_dist_sq));
  if (nq == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  KnnOut O{d_ids, d_dist_sq, d_counts, nullptr, 0};
  return knearest_launch<false>(t, d_q, nq, k, max_range, O, pick_stream(stream));
}

extern "C" pcgx_status pcgx_kdtree_knearest(const pcgx_kdtree *t, const float *q, int64_t nq, int32_t k, float max_range,
                                            int64_t *ids, float *dist_sq, int32_t *counts) {
  PCGX_API_CALL();
  PCGX_TRY(knearest_check("pcgx_kdtree_knearest", t, q, nq, k, max_range, ids, dist_sq));
  if (nq == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  const size_t slots = (size_t)nq * (size_t)k;
  float *d_q = nullptr, *d_d = nullptr;
  int32_t *d_i = nullptr, *d_c = nullptr;
  if (q) {
    PCGX_TRY(ha.alloc_n((size_t)nq * 3, &d_q));
    PCGX_TRY(staged_upload(d_q, q, (size_t)nq * 12, st));
  }
  PCGX_TRY(ha.alloc_n(slots, &d_i));
  PCGX_TRY(ha.alloc_n(slots, &d_d));
  if (counts) PCGX_TRY(ha.alloc_n((size_t)nq, &d_c));
  PCGX_TRY(pcgx_kdtree_knearest_dev(t, d_q, nq, k, max_range, d_i, d_d, d_c, st));
  // int32 on the device, int64 in the ABI (as Nearest's): widened in place from the back
  PCGX_TRY(staged_download(ids, d_i, slots * 4, st));
  const int32_t *narrow = reinterpret_cast<const int32_t *>(ids);
  for (size_t s = slots; s-- > 0;) ids[s] = (int64_t)narrow[s];
  PCGX_TRY(staged_download(dist_sq, d_d, slots * 4, st));
  if (counts) PCGX_TRY(staged_download(counts, d_c, (size_t)nq * 4, st));
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_kdtree_covariances_dev(const pcgx_kdtree *t, const float *d_q, int64_t nq, int32_t k,
                                                   float max_range, int32_t mode, float epsilon,
                                                   const float viewpoint[3], float *d_cov6, float *d_normals,
                                                   int32_t *d_counts, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(covariances_check("pcgx_kdtree_covariances_dev", t, d_q, nq, k, max_range, mode, epsilon, d_cov6));
  if (nq == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  CovOut O{d_cov6, d_normals, d_counts, nullptr, nullptr, 0.0f, 0.0f, 0.0f, epsilon, mode == PCGX_COV_PLANE ? 1 : 0};
  if (viewpoint) {
    O.vx = viewpoint[0];
    O.vy = viewpoint[1];
    O.vz = viewpoint[2];
  }
  return knearest_launch<false, true>(t, d_q, nq, k, max_range, O, pick_stream(stream));
}

extern "C" pcgx_status pcgx_kdtree_covariances(const pcgx_kdtree *t, const float *q, int64_t nq, int32_t k,
                                               float max_range, int32_t mode, float epsilon, const float viewpoint[3],
                                               float *cov6, float *normals, int32_t *counts) {
  PCGX_API_CALL();
  PCGX_TRY(covariances_check("pcgx_kdtree_covariances", t, q, nq, k, max_range, mode, epsilon, cov6));
  if (nq == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_q = nullptr, *d_c = nullptr, *d_n = nullptr;
  int32_t *d_k = nullptr;
  if (q) {
    PCGX_TRY(ha.alloc_n((size_t)nq * 3, &d_q));
    PCGX_TRY(staged_upload(d_q, q, (size_t)nq * 12, st));
  }
  PCGX_TRY(ha.alloc_n((size_t)nq * 6, &d_c));
  if (normals) PCGX_TRY(ha.alloc_n((size_t)nq * 3, &d_n));
  if (counts) PCGX_TRY(ha.alloc_n((size_t)nq, &d_k));
  PCGX_TRY(pcgx_kdtree_covariances_dev(t, d_q, nq, k, max_range, mode, epsilon, viewpoint, d_c, d_n, d_k, st));
  PCGX_TRY(staged_download(cov6, d_c, (size_t)nq * 24, st));
  if (normals) PCGX_TRY(staged_download(normals, d_n, (size_t)nq * 12, st));
  if (counts) PCGX_TRY(staged_download(counts, d_k, (size_t)nq * 4, st));
  return PCGX_OK;
}
