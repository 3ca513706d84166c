// rays.hip -- ray queries over a tree: the first point along each ray and how often each point was pierced (extension:
// no reference parity; include/pcgx.h, "ray queries").
//
// The members of a ray are the points inside a thin tube around it (ray_terms.h: the float64 member test).  They are
// found through the shared enumeration (radius_visit.h), on each of the three kinds of handle (grid, forced walk,
// patched tree after DeletePoint): the ray's range, clipped to the box of the tree's finite points, is cut into slabs,
// and each slab is one ball query whose candidates are kept where the member test passes and the slab owns their `a`
// (ray_terms.h: the cover and its proof).
//   ray_kernel   a wave per ray (a workgroup is one wave, kRangeWalkBlock, as the visitor requires).  Lane l takes slab
//                64 j + l of round j; all 64 lanes call radius_visit every round, live == false where a lane has no
//                slab, and serve the fat rows' shares with the owner's slab.  First hit: each lane keeps its best
//                (a, id), the wave reduces by shuffles after a round and leaves at the first round with a hit -- slabs
//                are in order of a, so nothing later can beat it.  Pierce: every round, atomicAdd on counts[id].
//   ray_scan_kernel  a tree with a NaN or infinite coordinate: a wave per ray over all points (see there).
// A minimum under a total order and an integer sum over a set: the result is a property of the point set and the rays,
// not of the order of the visit or of how the slabs fall.
#include <math.h>
#include <stdlib.h>

#include <mutex>

#include "radius_visit.h"
#include "ray_terms.h"

namespace pcgx {

constexpr int kRayBlock = kRangeWalkBlock;  // one wave per workgroup: the walks' LDS frame stacks are [level][64]

struct RayIn {
  const float *origins;     // [3 nr]
  const float *directions;  // [3 nr]
  const float *s_min;       // [nr] or NULL: 0
  const float *s_max;       // [nr] or NULL: +inf
  int64_t nr;
};

struct RayOut {
  int32_t *ids;     // first hit: [nr]
  double *along;    // [nr] or NULL
  double *off_sq;   // [nr] or NULL
  int32_t *counts;  // pierce: [Len()], added to
};

template <int kSrc, bool kPierce>
__global__ __launch_bounds__(kRayBlock) void ray_kernel(GridView g, TreeView tv, XTreeView xv, RayIn in, RayBox box,
                                                        float rho, float target, RayOut out, int64_t guard) {
  extern __shared__ uint32_t s_stack[];
  const int64_t ray = (int64_t)xcd_tile(blockIdx.x, (uint32_t)in.nr);
  if (ray >= in.nr) return;  // (the whole wave)
  const int lane = (int)(threadIdx.x & 63u);
  const Ray r = ray_make(in.origins[3 * ray], in.origins[3 * ray + 1], in.origins[3 * ray + 2], in.directions[3 * ray],
                         in.directions[3 * ray + 1], in.directions[3 * ray + 2], in.s_min ? in.s_min[ray] : 0.0f,
                         in.s_max ? in.s_max[ray] : __builtin_inff(), rho);
  double a0, a1;
  const bool some = ray_clip(r, box, rho, a0, a1);
  const int32_t K = some ? ray_slabs(r, a0, a1, target) : 0;
  const float bound = some ? ray_bound(r, box, rho, a0, a1, K) : 0.0f;
  double best_a = 0.0, best_cc = 0.0;
  int32_t best_id = -1;
  // the record p, reported by the ball of slab k
  auto consider = [&](const float4 &p, const int32_t k) {
    double a, cc;
    if (!ray_member(r, p.x, p.y, p.z, a, cc) || !ray_in_slab(a, a0, a1, k, K)) return;
    const int32_t id = (int32_t)__float_as_uint(p.w);
    if constexpr (kPierce) {
      atomicAdd(out.counts + id, 1);
    } else if (ray_beats(a, id, best_a, best_id)) {
      best_a = a, best_cc = cc, best_id = id;
    }
  };
  for (int32_t base = 0; base < K; base += 64) {  // uniform
    const int32_t k = base + lane;
    const bool live = k < K;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f;
    if (live) ray_centre(r, box, a0, a1, k, K, cx, cy, cz);
    radius_visit<kSrc>(
        RadiusViews{g, tv, xv, guard}, s_stack + threadIdx.x, kRayBlock, cx, cy, cz, bound, live,
        [&](const float4 &p, float) { consider(p, k); },
        [&](int owner, float, float, float, auto rows) {  // a share of the owner's fat row is tested for the owner's slab
          const int32_t ok = __shfl(k, owner);
          rows([&](const float4 &p, float) { consider(p, ok); });
        });
    if constexpr (!kPierce) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const double oa = __shfl_xor(best_a, m), occ = __shfl_xor(best_cc, m);
        const int32_t oid = __shfl_xor(best_id, m);
        if (ray_beats(oa, oid, best_a, best_id)) best_a = oa, best_cc = occ, best_id = oid;
      }
      if (best_id >= 0) break;  // uniform: every lane holds the winner
    }
  }
  if constexpr (!kPierce) {
    if (lane == 0) {
      out.ids[ray] = best_id;
      if (out.along) out.along[ray] = best_a;
      if (out.off_sq) out.off_sq[ray] = best_cc;
    }
  }
}

// A tree with a NaN or infinite coordinate among its points: the reference's build has no consistent order for a NaN,
// its walk (which the enumeration reproduces) may pass a finite point by, and Range's set there is "what the reference
// finds"; an infinite one leaves no box to clip to.  A ray's members are defined by the points alone, so on such a handle
// a wave tests its ray against every point: exact, and as slow as it sounds.  pts by id; deleted[id] != 0: not live
// (NULL: nothing deleted).
template <bool kPierce>
__global__ __launch_bounds__(kRayBlock) void ray_scan_kernel(const float *__restrict__ pts,
                                                             const uint8_t *__restrict__ deleted, int64_t n, RayIn in,
                                                             float rho, RayOut out) {
  const int64_t ray = (int64_t)blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const Ray r = ray_make(in.origins[3 * ray], in.origins[3 * ray + 1], in.origins[3 * ray + 2], in.directions[3 * ray],
                         in.directions[3 * ray + 1], in.directions[3 * ray + 2], in.s_min ? in.s_min[ray] : 0.0f,
                         in.s_max ? in.s_max[ray] : __builtin_inff(), rho);
  double best_a = 0.0, best_cc = 0.0;
  int32_t best_id = -1;
  for (int64_t i = lane; i < n; i += 64) {
    double a, cc;
    if ((deleted && deleted[i]) || !ray_member(r, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], a, cc)) continue;
    if constexpr (kPierce) {
      atomicAdd(out.counts + i, 1);
    } else if (ray_beats(a, (int32_t)i, best_a, best_id)) {
      best_a = a, best_cc = cc, best_id = (int32_t)i;
    }
  }
  if constexpr (!kPierce) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double oa = __shfl_xor(best_a, m), occ = __shfl_xor(best_cc, m);
      const int32_t oid = __shfl_xor(best_id, m);
      if (ray_beats(oa, oid, best_a, best_id)) best_a = oa, best_cc = occ, best_id = oid;
    }
    if (lane == 0) {
      out.ids[ray] = best_id;
      if (out.along) out.along[ray] = best_a;
      if (out.off_sq) out.off_sq[ray] = best_cc;
    }
  }
}

template <bool kPierce>
pcgx_status ray_scan_enqueue(const pcgx_kdtree *tc, const RayIn &in, float rho, const RayOut &out, hipStream_t st) {
  pcgx_kdtree *t = const_cast<pcgx_kdtree *>(tc);
  std::lock_guard<std::mutex> lock(t->mu);
  const int64_t n = t->n;
  float *d_pts = nullptr;
  uint8_t *d_deleted = nullptr;
  PCGX_TRY(ctx().arena.alloc_n((size_t)n * 3, &d_pts));
  PCGX_TRY(staged_upload(d_pts, t->points.data(), (size_t)n * 12, st));
  if (t->n_deleted > 0) {
    PCGX_TRY(ctx().arena.alloc_n((size_t)n, &d_deleted));
    PCGX_TRY(staged_upload(d_deleted, t->deleted.data(), (size_t)n, st));
  }
  hipLaunchKernelGGL(ray_scan_kernel<kPierce>, dim3((unsigned)in.nr), dim3(kRayBlock), 0, st, d_pts, d_deleted, n, in, rho,
                     out);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

template <int kSrc, bool kPierce>
void ray_launch(const pcgx_kdtree *t, const TreeView &tv, const XTreeView &xv, const RayIn &in, const RayBox &box,
                float rho, float target, const RayOut &out, size_t stack_bytes, hipStream_t st) {
  const dim3 grid(xcd_grid((unsigned)in.nr)), block(kRayBlock);
  const GridView g = kSrc == kRangeGrid ? t->grid : GridView{};
  hipLaunchKernelGGL((ray_kernel<kSrc, kPierce>), grid, block, stack_bytes, st, g, tv, xv, in, box, rho, target, out,
                     xwalk_guard(t->n));
}

// The box of the handle's finite points (deleted ones too: the box may only be too wide), made once per handle.
// (m3c2.hip's cylinders clip to it too.)
RayBox ray_box(const pcgx_kdtree *tc) {
  pcgx_kdtree *t = const_cast<pcgx_kdtree *>(tc);
  std::lock_guard<std::mutex> lock(t->mu);
  if (t->ray_box_state == 0) {
    bool any = false;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    const float *pp = t->points.data();
    for (int64_t i = 0; i < t->n; i++) {
      const float *p = pp + 3 * i;
      if (!(ray_finite(p[0]) && ray_finite(p[1]) && ray_finite(p[2]))) {
        t->ray_all_finite = false;
        continue;
      }
      for (int k = 0; k < 3; k++) {
        lo[k] = !any || p[k] < lo[k] ? p[k] : lo[k];
        hi[k] = !any || p[k] > hi[k] ? p[k] : hi[k];
      }
      any = true;
    }
    for (int k = 0; k < 3; k++) t->ray_lo[k] = lo[k], t->ray_hi[k] = hi[k];
    t->ray_box_state = any ? 1 : 2;
  }
  RayBox b;
  for (int k = 0; k < 3; k++) b.lo[k] = t->ray_lo[k], b.hi[k] = t->ray_hi[k];
  b.any = t->ray_box_state == 1;
  return b;
}

// nr > 0, everything device resident
template <bool kPierce>
pcgx_status rays_enqueue(const pcgx_kdtree *t, const RayIn &in, float rho, const RayOut &out, hipStream_t st) {
  const RayBox box = ray_box(t);
  if (!t->ray_all_finite) return ray_scan_enqueue<kPierce>(t, in, rho, out, st);
  const RangeSrc src = range_source(t);  // as pcgx_kdtree_range_count takes it
  XTreeView xv{};
  if (src == kRangeXWalk) PCGX_TRY(xtree_view(t, &xv, st));
  const TreeView tv = t->view();
  // a slab is about as long as the tube is wide, and no shorter than a cell of the grid, whose rows a ball reads whole
  float target = 2.0f * rho;
  if (src == kRangeGrid && t->grid.h > target) target = t->grid.h;
  if (!(target < __builtin_inff())) target = 3.0e38f;
  if (src == kRangeXWalk) ray_launch<kRangeXWalk, kPierce>(t, tv, xv, in, box, rho, target, out, xwalk_stack_bytes(xv, kRayBlock), st);
  else if (src == kRangeGrid) ray_launch<kRangeGrid, kPierce>(t, tv, xv, in, box, rho, target, out, 0, st);
  else ray_launch<kRangeWalk, kPierce>(t, tv, xv, in, box, rho, target, out, walk_stack_bytes(tv, kRayBlock), st);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kRayMaxRays = 0x7ffffff0;    // a workgroup per ray
constexpr int64_t kRayMaxPoints = 0x7fffffff;  // ids are int32 on the device

// out: ids, or counts (which an empty tree does not need)
pcgx_status rays_check(const char *fn, const pcgx_kdtree *t, float rho, const void *origins, const void *directions,
                       int64_t nr, const void *out, bool is_counts) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!(rho > 0.0f && rho < __builtin_inff())) return fail(PCGX_E_INVALID, "%s: radius must be finite and > 0", fn);
  if (nr < 0 || nr > kRayMaxRays) return fail(PCGX_E_INVALID, "%s: nr must be 0 .. 2^31 - 16", fn);
  if (t->n > kRayMaxPoints) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points", fn);
  if (nr > 0 && (!origins || !directions || (!out && !(is_counts && t->n == 0))))
    return fail(PCGX_E_INVALID, "%s: NULL origins, directions or output", fn);
  if (t->n > 0 && nr > 0) {
    const RayBox b = ray_box(t);
    for (int k = 0; k < 3; k++)
      if (b.any && !(b.hi[k] - b.lo[k] < kRayMaxExtent))
        return fail(PCGX_E_INVALID, "%s: the tree's finite points span 2^62 or more along an axis", fn);
  }
  return PCGX_OK;
}

// the rays of a host call on the device
pcgx_status rays_upload(Arena &ha, const float *origins, const float *directions, const float *s_min, const float *s_max,
                        int64_t nr, RayIn *in, hipStream_t st) {
  float *d_o = nullptr, *d_d = nullptr, *d_lo = nullptr, *d_hi = nullptr;
  PCGX_TRY(ha.alloc_n((size_t)nr * 3, &d_o));
  PCGX_TRY(ha.alloc_n((size_t)nr * 3, &d_d));
  PCGX_TRY(staged_upload(d_o, origins, (size_t)nr * 12, st));
  PCGX_TRY(staged_upload(d_d, directions, (size_t)nr * 12, st));
  if (s_min) {
    PCGX_TRY(ha.alloc_n((size_t)nr, &d_lo));
    PCGX_TRY(staged_upload(d_lo, s_min, (size_t)nr * 4, st));
  }
  if (s_max) {
    PCGX_TRY(ha.alloc_n((size_t)nr, &d_hi));
    PCGX_TRY(staged_upload(d_hi, s_max, (size_t)nr * 4, st));
  }
  *in = RayIn{d_o, d_d, d_lo, d_hi, nr};
  return PCGX_OK;
}

}  // namespace

extern "C" pcgx_status pcgx_kdtree_raycast_dev(const pcgx_kdtree *t, const float *d_origins, const float *d_directions,
                                               const float *d_s_min, const float *d_s_max, int64_t nr, float radius,
                                               int32_t *d_ids, double *d_along, double *d_off_sq, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(rays_check("pcgx_kdtree_raycast_dev", t, radius, d_origins, d_directions, nr, d_ids, false));
  if (nr == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  PCGX_TRY(ctx().arena.begin(st));
  // (an empty tree too: its box holds nothing, no slab is made and every ray is written as a miss)
  return rays_enqueue<false>(t, RayIn{d_origins, d_directions, d_s_min, d_s_max, nr}, radius,
                             RayOut{d_ids, d_along, d_off_sq, nullptr}, st);
}

extern "C" pcgx_status pcgx_kdtree_raycast(const pcgx_kdtree *t, const float *origins, const float *directions,
                                           const float *s_min, const float *s_max, int64_t nr, float radius, int64_t *ids,
                                           double *along, double *off_sq) {
  PCGX_API_CALL();
  PCGX_TRY(rays_check("pcgx_kdtree_raycast", t, radius, origins, directions, nr, ids, false));
  if (nr == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  RayIn in;
  PCGX_TRY(rays_upload(ha, origins, directions, s_min, s_max, nr, &in, st));
  int32_t *d_ids = nullptr;
  double *d_along = nullptr, *d_off = nullptr;
  PCGX_TRY(ha.alloc_n((size_t)nr, &d_ids));
  if (along) PCGX_TRY(ha.alloc_n((size_t)nr, &d_along));
  if (off_sq) PCGX_TRY(ha.alloc_n((size_t)nr, &d_off));
  PCGX_TRY(pcgx_kdtree_raycast_dev(t, in.origins, in.directions, in.s_min, in.s_max, nr, radius, d_ids, d_along, d_off, st));
  if (along) PCGX_TRY(staged_download(along, d_along, (size_t)nr * 8, st));
  if (off_sq) PCGX_TRY(staged_download(off_sq, d_off, (size_t)nr * 8, st));
  RawVector<int32_t> h((size_t)nr);
  PCGX_TRY(staged_download(h.data(), d_ids, (size_t)nr * 4, st));
  for (int64_t i = 0; i < nr; i++) ids[i] = h[(size_t)i];
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_kdtree_ray_pierce_dev(const pcgx_kdtree *t, const float *d_origins, const float *d_directions,
                                                  const float *d_s_min, const float *d_s_max, int64_t nr, float radius,
                                                  int32_t *d_counts, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(rays_check("pcgx_kdtree_ray_pierce_dev", t, radius, d_origins, d_directions, nr, d_counts, true));
  if (nr == 0 || t->n == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  PCGX_TRY(ctx().arena.begin(st));
  return rays_enqueue<true>(t, RayIn{d_origins, d_directions, d_s_min, d_s_max, nr}, radius,
                            RayOut{nullptr, nullptr, nullptr, d_counts}, st);
}

extern "C" pcgx_status pcgx_kdtree_ray_pierce(const pcgx_kdtree *t, const float *origins, const float *directions,
                                              const float *s_min, const float *s_max, int64_t nr, float radius,
                                              int32_t *counts) {
  PCGX_API_CALL();
  PCGX_TRY(rays_check("pcgx_kdtree_ray_pierce", t, radius, origins, directions, nr, counts, true));
  const int64_t n = t->n;
  if (n == 0) return PCGX_OK;
  if (nr == 0) {
    for (int64_t i = 0; counts && i < n; i++) counts[i] = 0;
    return PCGX_OK;
  }
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  RayIn in;
  PCGX_TRY(rays_upload(ha, origins, directions, s_min, s_max, nr, &in, st));
  int32_t *d_counts = nullptr;
  PCGX_TRY(ha.alloc_n((size_t)n, &d_counts));
  PCGX_HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)n * 4, st));
  PCGX_TRY(pcgx_kdtree_ray_pierce_dev(t, in.origins, in.directions, in.s_min, in.s_max, nr, radius, d_counts, st));
  return staged_download(counts, d_counts, (size_t)n * 4, st);
}
