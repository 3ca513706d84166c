// m3c2.hip -- cylinder statistics over a tree, and M3C2's finish on the statistics of two epochs (extension: no
// reference parity; include/pcgx.h, "cylinder statistics" and "M3C2").
//
// The members of a cylinder are the points inside a tube around its axis, cut at both ends (m3c2_terms.h: the float64
// member test).  They are found as the ray queries find theirs (rays.hip, ray_terms.h: clip, slabs, one ball query per
// slab, the cover's proof), on each of the three kinds of handle.  What differs is what is kept -- the count and the
// sums of a and a.a per cylinder -- and how lanes are dealt: a cylinder has 2 L / max(2 rho, h) slabs, a handful, not
// a LiDAR ray's thousands.
//   cyl_kernel<kSrc, W>  W lanes per cylinder, 64 / W cylinders per wave (a workgroup is one wave, kRangeWalkBlock, as
//                the visitor requires): lane l takes slab l % W (+ W per round) of cylinder slot l / W.  All 64 lanes
//                call radius_visit every round under the wave's largest ray_bound (the visitor shares fat rows out
//                under the calling lane's bound; a wider bound only adds candidates, the member test and ray_in_slab
//                decide).  A lane adds the members its slab owns in the order of the visit; a fat row's share is added
//                per lane, reduced over the wave by xor shuffles and added by the owner; at the end a cylinder's W
//                lanes are reduced by xor shuffles and the slot's first lane writes.  Every step is a fixed order: the
//                same handle, arguments and build give the same bits.  No float atomics, no temporaries.
//   cyl_scan_kernel  a tree with a NaN or infinite coordinate: a wave per cylinder over all points (ray_scan_kernel).
//   m3c2_finish_kernel  a thread per core: m3c2_terms.h's m3c2_finish.
// W: the host takes the smallest of 8, 16, 64 that is at least cyl_slab_bound (m3c2_terms.h); the kernel loops over
// rounds of W slabs whatever W is, so a bound that were too small would cost time and never a member.
#include <math.h>
#include <stdlib.h>

#include <mutex>

#include "m3c2_terms.h"
#include "radius_visit.h"

namespace pcgx {

RayBox ray_box(const pcgx_kdtree *tc);  // rays.hip

constexpr int kCylBlock = kRangeWalkBlock;  // one wave per workgroup: the walks' LDS frame stacks are [level][64]
constexpr int kFinishBlock = 256;

struct CylIn {
  const float *cores;  // [3 m]
  const float *axes;   // [3 m]
  int64_t m;
};

struct CylOut {
  int32_t *counts;  // [m]
  double *sums;     // [2 m]: S1, S2
};

// cylinder i; beyond m: one with dd == 0, which has no members
__device__ __forceinline__ Cyl cyl_load(const CylIn &in, const int64_t i, const float rho, const float half_length) {
  if (i >= in.m) return cyl_make(0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, rho, half_length);
  return cyl_make(in.cores[3 * i], in.cores[3 * i + 1], in.cores[3 * i + 2], in.axes[3 * i], in.axes[3 * i + 1],
                  in.axes[3 * i + 2], rho, half_length);
}

// the record p, reported by the ball of slab k of K over [a0, a1]
__device__ __forceinline__ void cyl_consider(const Cyl &c, const double a0, const double a1, const int32_t k,
                                             const int32_t K, const float4 &p, int32_t &n, double &s1, double &s2) {
  double a, cc;
  if (!cyl_member(c, p.x, p.y, p.z, a, cc) || !ray_in_slab(a, a0, a1, k, K)) return;
  n += 1;
  s1 += a;
  s2 += a * a;
}

template <int kSrc, int W>
__global__ __launch_bounds__(kCylBlock) void cyl_kernel(GridView g, TreeView tv, XTreeView xv, CylIn in, RayBox box,
                                                        float rho, float half_length, float target, CylOut out,
                                                        int64_t guard) {
  extern __shared__ uint32_t s_stack[];
  constexpr int kSlots = 64 / W;
  const uint32_t ntiles = (uint32_t)((in.m + kSlots - 1) / kSlots);
  const uint32_t tile = xcd_tile(blockIdx.x, ntiles);
  if (tile >= ntiles) return;  // (the whole wave)
  const int lane = (int)(threadIdx.x & 63u);
  const int slot = lane / W, sl = lane % W;
  const int64_t first = (int64_t)tile * kSlots;
  const Cyl c = cyl_load(in, first + slot, rho, half_length);
  double a0, a1;
  const bool some = ray_clip(c.r, box, rho, a0, a1);
  const int32_t K = some ? ray_slabs(c.r, a0, a1, target) : 0;
  float bound = some ? ray_bound(c.r, box, rho, a0, a1, K) : 0.0f;
  int32_t k_wave = K;  // the rounds are the wave's
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    bound = fmaxf(bound, __shfl_xor(bound, m));
    k_wave = max(k_wave, __shfl_xor(k_wave, m));
  }
  int32_t n = 0;
  double s1 = 0.0, s2 = 0.0;
  for (int32_t base = 0; base < k_wave; base += W) {  // uniform
    const int32_t k = base + sl;
    const bool live = k < K;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f;
    if (live) ray_centre(c.r, box, a0, a1, k, K, cx, cy, cz);
    radius_visit<kSrc>(
        RadiusViews{g, tv, xv, guard}, s_stack + threadIdx.x, kCylBlock, cx, cy, cz, bound, live,
        [&](const float4 &p, float) { cyl_consider(c, a0, a1, k, K, p, n, s1, s2); },
        [&](int owner, float, float, float, auto rows) {  // a share of the owner's fat row, for the owner's cylinder and slab
          const Cyl oc = cyl_load(in, first + owner / W, rho, half_length);
          const double oa0 = __shfl(a0, owner), oa1 = __shfl(a1, owner);
          const int32_t oK = __shfl(K, owner), ok = base + owner % W;
          int32_t pn = 0;
          double p1 = 0.0, p2 = 0.0;
          rows([&](const float4 &p, float) { cyl_consider(oc, oa0, oa1, ok, oK, p, pn, p1, p2); });
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) {
            pn += __shfl_xor(pn, m);
            p1 += __shfl_xor(p1, m);
            p2 += __shfl_xor(p2, m);
          }
          if (lane == owner) n += pn, s1 += p1, s2 += p2;
        });
  }
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) {
    n += __shfl_xor(n, m);
    s1 += __shfl_xor(s1, m);
    s2 += __shfl_xor(s2, m);
  }
  if (sl == 0 && first + slot < in.m) {
    out.counts[first + slot] = n;
    out.sums[2 * (first + slot)] = s1;
    out.sums[2 * (first + slot) + 1] = s2;
  }
}

// A tree with a NaN or infinite coordinate among its points (rays.hip, ray_scan_kernel: why): a wave tests its cylinder
// against every point.  pts by id; deleted[id] != 0: not live (NULL: nothing deleted).
__global__ __launch_bounds__(kCylBlock) void cyl_scan_kernel(const float *__restrict__ pts,
                                                             const uint8_t *__restrict__ deleted, int64_t n, CylIn in,
                                                             float rho, float half_length, CylOut out) {
  const int64_t i = (int64_t)blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const Cyl c = cyl_load(in, i, rho, half_length);
  int32_t cn = 0;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t j = lane; j < n; j += 64) {
    double a, cc;
    if ((deleted && deleted[j]) || !cyl_member(c, pts[3 * j], pts[3 * j + 1], pts[3 * j + 2], a, cc)) continue;
    cn += 1;
    s1 += a;
    s2 += a * a;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    cn += __shfl_xor(cn, m);
    s1 += __shfl_xor(s1, m);
    s2 += __shfl_xor(s2, m);
  }
  if (lane == 0) {
    out.counts[i] = cn;
    out.sums[2 * i] = s1;
    out.sums[2 * i + 1] = s2;
  }
}

__global__ __launch_bounds__(kFinishBlock) void m3c2_finish_kernel(const float *__restrict__ axes,
                                                                   const int32_t *__restrict__ n1,
                                                                   const double *__restrict__ sums1,
                                                                   const int32_t *__restrict__ n2,
                                                                   const double *__restrict__ sums2, int64_t m,
                                                                   double registration_error, int32_t min_count,
                                                                   double *__restrict__ distance, double *__restrict__ lod,
                                                                   uint8_t *__restrict__ significant) {
  const int64_t i = (int64_t)blockIdx.x * kFinishBlock + threadIdx.x;
  if (i >= m) return;
  const M3C2Value v = m3c2_finish(axes[3 * i], axes[3 * i + 1], axes[3 * i + 2], n1[i], sums1[2 * i], sums1[2 * i + 1],
                                  n2[i], sums2[2 * i], sums2[2 * i + 1], registration_error, min_count);
  distance[i] = v.distance;
  lod[i] = v.lod;
  significant[i] = v.significant;
}

static pcgx_status cyl_scan_enqueue(const pcgx_kdtree *tc, const CylIn &in, float rho, float half_length,
                                    const CylOut &out, hipStream_t st) {
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
  hipLaunchKernelGGL(cyl_scan_kernel, dim3((unsigned)in.m), dim3(kCylBlock), 0, st, d_pts, d_deleted, n, in, rho,
                     half_length, out);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

template <int kSrc, int W>
static void cyl_launch(const pcgx_kdtree *t, const TreeView &tv, const XTreeView &xv, const CylIn &in, const RayBox &box,
                       float rho, float half_length, float target, const CylOut &out, size_t stack_bytes,
                       hipStream_t st) {
  constexpr int kSlots = 64 / W;
  const dim3 grid(xcd_grid((unsigned)((in.m + kSlots - 1) / kSlots))), block(kCylBlock);
  const GridView g = kSrc == kRangeGrid ? t->grid : GridView{};
  hipLaunchKernelGGL((cyl_kernel<kSrc, W>), grid, block, stack_bytes, st, g, tv, xv, in, box, rho, half_length, target,
                     out, xwalk_guard(t->n));
}

template <int kSrc>
static void cyl_launch_lanes(int lanes, const pcgx_kdtree *t, const TreeView &tv, const XTreeView &xv, const CylIn &in,
                             const RayBox &box, float rho, float half_length, float target, const CylOut &out,
                             size_t stack_bytes, hipStream_t st) {
  if (lanes == 8) cyl_launch<kSrc, 8>(t, tv, xv, in, box, rho, half_length, target, out, stack_bytes, st);
  else if (lanes == 16) cyl_launch<kSrc, 16>(t, tv, xv, in, box, rho, half_length, target, out, stack_bytes, st);
  else cyl_launch<kSrc, 64>(t, tv, xv, in, box, rho, half_length, target, out, stack_bytes, st);
}

// Lanes per cylinder: the smallest of 8, 16, 64 that holds every slab of a cylinder in one round (64 beyond: rounds).
// PCGX_CYL_LANES=16 / 64: a wider choice than that (measurements: tools/m3c2_probe.py); a narrower one is ignored.
static int cyl_lanes(const float half_length, const float target) {
  const double kb = cyl_slab_bound(half_length, target);
  int lanes = kb <= 8.0 ? 8 : kb <= 16.0 ? 16 : 64;  // (a NaN: 64)
  const char *e = getenv("PCGX_CYL_LANES");
  const int forced = e ? atoi(e) : 0;
  if ((forced == 16 || forced == 64) && forced > lanes) lanes = forced;
  return lanes;
}

// m > 0, everything device resident
static pcgx_status cyl_enqueue(const pcgx_kdtree *t, const CylIn &in, float rho, float half_length, const CylOut &out,
                               hipStream_t st) {
  const RayBox box = ray_box(t);
  if (!t->ray_all_finite) return cyl_scan_enqueue(t, in, rho, half_length, out, st);
  const RangeSrc src = range_source(t);  // as pcgx_kdtree_range_count takes it
  XTreeView xv{};
  if (src == kRangeXWalk) PCGX_TRY(xtree_view(t, &xv, st));
  const TreeView tv = t->view();
  // a slab is about as long as the tube is wide, and no shorter than a cell of the grid, whose rows a ball reads whole
  float target = 2.0f * rho;
  if (src == kRangeGrid && t->grid.h > target) target = t->grid.h;
  if (!(target < __builtin_inff())) target = 3.0e38f;
  const int lanes = cyl_lanes(half_length, target);
  if (src == kRangeXWalk)
    cyl_launch_lanes<kRangeXWalk>(lanes, t, tv, xv, in, box, rho, half_length, target, out, xwalk_stack_bytes(xv, kCylBlock), st);
  else if (src == kRangeGrid)
    cyl_launch_lanes<kRangeGrid>(lanes, t, tv, xv, in, box, rho, half_length, target, out, 0, st);
  else
    cyl_launch_lanes<kRangeWalk>(lanes, t, tv, xv, in, box, rho, half_length, target, out, walk_stack_bytes(tv, kCylBlock), st);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kCylMaxCylinders = 0x7ffffff0;  // a workgroup per cylinder at most (the scan; W = 64)
constexpr int64_t kCylMaxPoints = 0x7fffffff;     // counts are int32

pcgx_status cyl_check(const char *fn, const pcgx_kdtree *t, float rho, float half_length, const void *cores,
                      const void *axes, int64_t m, const void *counts, const void *sums) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!(rho > 0.0f && rho < __builtin_inff())) return fail(PCGX_E_INVALID, "%s: radius must be finite and > 0", fn);
  if (!(half_length > 0.0f && half_length < __builtin_inff()))
    return fail(PCGX_E_INVALID, "%s: half_length must be finite and > 0", fn);
  if (m < 0 || m > kCylMaxCylinders) return fail(PCGX_E_INVALID, "%s: m must be 0 .. 2^31 - 16", fn);
  if (t->n > kCylMaxPoints) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points", fn);
  if (m > 0 && (!cores || !axes || !counts || !sums)) return fail(PCGX_E_INVALID, "%s: NULL cores, axes, counts or sums", fn);
  if (t->n > 0 && m > 0) {
    const RayBox b = ray_box(t);
    for (int k = 0; k < 3; k++)
      if (b.any && !(b.hi[k] - b.lo[k] < kRayMaxExtent))
        return fail(PCGX_E_INVALID, "%s: the tree's finite points span 2^62 or more along an axis", fn);
  }
  return PCGX_OK;
}

pcgx_status finish_check(const char *fn, const void *axes, const void *n1, const void *s1, const void *n2, const void *s2,
                         int64_t m, double registration_error, int32_t min_count, const void *distance, const void *lod,
                         const void *significant) {
  if (m < 0 || m > kCylMaxPoints) return fail(PCGX_E_INVALID, "%s: m must be 0 .. 2^31 - 1", fn);
  if (!(registration_error >= 0.0)) return fail(PCGX_E_INVALID, "%s: registration_error must be >= 0", fn);
  if (min_count < 2) return fail(PCGX_E_INVALID, "%s: min_count must be >= 2", fn);
  if (m > 0 && (!axes || !n1 || !s1 || !n2 || !s2 || !distance || !lod || !significant))
    return fail(PCGX_E_INVALID, "%s: NULL array", fn);
  return PCGX_OK;
}

}  // namespace

extern "C" pcgx_status pcgx_kdtree_cylinder_stats_dev(const pcgx_kdtree *t, const float *d_cores, const float *d_axes,
                                                      int64_t m, float radius, float half_length, int32_t *d_counts,
                                                      double *d_sums, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(cyl_check("pcgx_kdtree_cylinder_stats_dev", t, radius, half_length, d_cores, d_axes, m, d_counts, d_sums));
  if (m == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  PCGX_TRY(ctx().arena.begin(st));
  // (an empty tree too: its box holds nothing, no slab is made and every cylinder is written as 0, 0, 0)
  return cyl_enqueue(t, CylIn{d_cores, d_axes, m}, radius, half_length, CylOut{d_counts, d_sums}, st);
}

extern "C" pcgx_status pcgx_kdtree_cylinder_stats(const pcgx_kdtree *t, const float *cores, const float *axes, int64_t m,
                                                  float radius, float half_length, int32_t *counts, double *sums) {
  PCGX_API_CALL();
  PCGX_TRY(cyl_check("pcgx_kdtree_cylinder_stats", t, radius, half_length, cores, axes, m, counts, sums));
  if (m == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_c = nullptr, *d_a = nullptr;
  int32_t *d_counts = nullptr;
  double *d_sums = nullptr;
  PCGX_TRY(ha.alloc_n((size_t)m * 3, &d_c));
  PCGX_TRY(ha.alloc_n((size_t)m * 3, &d_a));
  PCGX_TRY(ha.alloc_n((size_t)m, &d_counts));
  PCGX_TRY(ha.alloc_n((size_t)m * 2, &d_sums));
  PCGX_TRY(staged_upload(d_c, cores, (size_t)m * 12, st));
  PCGX_TRY(staged_upload(d_a, axes, (size_t)m * 12, st));
  PCGX_TRY(pcgx_kdtree_cylinder_stats_dev(t, d_c, d_a, m, radius, half_length, d_counts, d_sums, st));
  PCGX_TRY(staged_download(counts, d_counts, (size_t)m * 4, st));
  return staged_download(sums, d_sums, (size_t)m * 16, st);
}

extern "C" pcgx_status pcgx_m3c2_finish_dev(const float *d_axes, const int32_t *d_counts1, const double *d_sums1,
                                            const int32_t *d_counts2, const double *d_sums2, int64_t m,
                                            double registration_error, int32_t min_count, double *d_distance,
                                            double *d_lod, uint8_t *d_significant, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(finish_check("pcgx_m3c2_finish_dev", d_axes, d_counts1, d_sums1, d_counts2, d_sums2, m, registration_error,
                        min_count, d_distance, d_lod, d_significant));
  if (m == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  hipLaunchKernelGGL(m3c2_finish_kernel, dim3((unsigned)((m + kFinishBlock - 1) / kFinishBlock)), dim3(kFinishBlock), 0, st,
                     d_axes, d_counts1, d_sums1, d_counts2, d_sums2, m, registration_error, min_count, d_distance, d_lod,
                     d_significant);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_m3c2_finish(const float *axes, const int32_t *counts1, const double *sums1,
                                        const int32_t *counts2, const double *sums2, int64_t m,
                                        double registration_error, int32_t min_count, double *distance, double *lod,
                                        uint8_t *significant) {
  PCGX_API_CALL();
  PCGX_TRY(finish_check("pcgx_m3c2_finish", axes, counts1, sums1, counts2, sums2, m, registration_error, min_count,
                        distance, lod, significant));
  if (m == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_a = nullptr;
  int32_t *d_n1 = nullptr, *d_n2 = nullptr;
  double *d_s1 = nullptr, *d_s2 = nullptr, *d_dist = nullptr, *d_lod = nullptr;
  uint8_t *d_sig = nullptr;
  PCGX_TRY(ha.alloc_n((size_t)m * 3, &d_a));
  PCGX_TRY(ha.alloc_n((size_t)m, &d_n1));
  PCGX_TRY(ha.alloc_n((size_t)m, &d_n2));
  PCGX_TRY(ha.alloc_n((size_t)m * 2, &d_s1));
  PCGX_TRY(ha.alloc_n((size_t)m * 2, &d_s2));
  PCGX_TRY(ha.alloc_n((size_t)m, &d_dist));
  PCGX_TRY(ha.alloc_n((size_t)m, &d_lod));
  PCGX_TRY(ha.alloc_n((size_t)m, &d_sig));
  PCGX_TRY(staged_upload(d_a, axes, (size_t)m * 12, st));
  PCGX_TRY(staged_upload(d_n1, counts1, (size_t)m * 4, st));
  PCGX_TRY(staged_upload(d_n2, counts2, (size_t)m * 4, st));
  PCGX_TRY(staged_upload(d_s1, sums1, (size_t)m * 16, st));
  PCGX_TRY(staged_upload(d_s2, sums2, (size_t)m * 16, st));
  PCGX_TRY(pcgx_m3c2_finish_dev(d_a, d_n1, d_s1, d_n2, d_s2, m, registration_error, min_count, d_dist, d_lod, d_sig, st));
  PCGX_TRY(staged_download(distance, d_dist, (size_t)m * 8, st));
  PCGX_TRY(staged_download(lod, d_lod, (size_t)m * 8, st));
  return staged_download(significant, d_sig, (size_t)m * 1, st);
}
