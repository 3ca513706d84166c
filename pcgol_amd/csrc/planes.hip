// planes.hip -- plane segmentation: the plane most of the cloud agrees on, by sample consensus over the caller's samples,
// its inliers taken out, then the next one (extension: no reference parity; include/pcgx.h, "planes").  The contract of
// pose.hip: the caller draws every random word, one call fits and scores all hypotheses, the first best wins.  The rounds
// -- the device words they hand on, the select, the ordered compaction of the points that are left, the round end -- are
// consensus_peel.h's, over PlaneModel; a round's records are 16 bytes a point, 16 more with normals.  This file's own:
//   planes_fit_kernel         a lane per hypothesis: plane_terms.h's plane_hypothesis -> status and plane, count 0.
//   planes_count_kernel       the hot one, hypotheses x points: pose_count_kernel's shape.  One wave per workgroup, TWO
//                             hypotheses per lane, their four numbers as packed float32 pairs (each half rounded on its
//                             own: the bits of two plain operations), the point record wave-uniform through scalar
//                             loads, blockIdx.y over chunks of the list, an integer atomicAdd per lane at the end.  No LDS.
//   planes_refit_kernel       one lane: plane_terms.h's plane_refit from group geometry's answer (group_stats.hip's own
//                             kernels, enqueued on the candidate inlier list with its size in a device word).
// Integer atomics only: the same input gives the same bits on every call, whatever the split.
#include <math.h>
#include <string.h>

#include "consensus_peel.h"
#include "group_list.h"

namespace pcgx {

constexpr int kPlBlock = kPeelBlock, kPlTile = kPeelTile;
static_assert(kPlaneNotRun == kPeelNotRun && kPlaneOk == kPeelOk, "the status codes the rounds read");

typedef float plane_f2 __attribute__((ext_vector_type(2)));

// A record is the plane's four numbers; an inlier lies nearer than max_dist and, where there are normals, its normal
// agrees with the plane's.
struct PlaneModel {
  static constexpr int kRec = 4, kMinSample = 3;
  struct Test {
    float max_dist, min_normal_cos;
  };
  struct Rec {
    float v[4];
  };
  static __device__ __forceinline__ Rec load(const float *rec, const Test &) { return Rec{{rec[0], rec[1], rec[2], rec[3]}}; }
  static __device__ __forceinline__ bool inlier(const Rec &pl, const Test &T, float4 p, const float4 *__restrict__ N,
                                                int64_t i) {
    bool in = plane_near(pl.v, p.x, p.y, p.z, T.max_dist);
    if (N) {
      const float4 m = N[i];
      in = in && plane_normal_agrees(pl.v, m.x, m.y, m.z, T.min_normal_cos);
    }
    return in;
  }
};
typedef PeelState<PlaneModel::kRec> PlaneState;

__global__ __launch_bounds__(256) void planes_fit_kernel(const PlaneState *__restrict__ S, const float4 *__restrict__ P,
                                                         const uint32_t *__restrict__ samples, int64_t n_hyp, PlaneAxis ax,
                                                         int32_t *__restrict__ status, int32_t *__restrict__ counts,
                                                         float *__restrict__ hyp) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n_hyp) return;
  float pl[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int32_t st = kPlaneNotRun;
  if (S->run) {
    const uint32_t R = (uint32_t)S->R;
    const uint32_t i0 = pose_sample_index(samples[3 * h], R), i1 = pose_sample_index(samples[3 * h + 1], R),
                   i2 = pose_sample_index(samples[3 * h + 2], R);
    const float4 p0 = P[i0], p1 = P[i1], p2 = P[i2];
    st = plane_hypothesis(i0, i1, i2, &p0.x, &p1.x, &p2.x, ax, pl);
  }
  status[h] = st;
  counts[h] = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) hyp[4 * h + k] = pl[k];  // (the caller's array: no alignment beyond a float's)
}

template <bool kNormals>
__global__ __launch_bounds__(kPlBlock) void planes_count_kernel(const PlaneState *__restrict__ S, const float4 *__restrict__ P,
                                                                const float4 *__restrict__ N, int64_t n_hyp,
                                                                const int32_t *__restrict__ status,
                                                                const float *__restrict__ hyp, float max_dist,
                                                                float min_normal_cos, int32_t chunk,
                                                                int32_t *__restrict__ counts) {
  if (!S->run) return;  // (uniform)
  const int64_t h0 = (int64_t)blockIdx.x * kPlTile + threadIdx.x, h1 = h0 + kPlBlock;
  const bool ok0 = h0 < n_hyp && status[h0] == kPlaneOk, ok1 = h1 < n_hyp && status[h1] == kPlaneOk;
  if (__ballot(ok0 || ok1) == 0ull) return;  // (wave-uniform)
  const int64_t len = S->R;
  const int64_t k0 = (int64_t)blockIdx.y * chunk;
  if (k0 >= len) return;
  const int64_t k1 = k0 + chunk < len ? k0 + chunk : len;
  const float *a = hyp + 4 * (h0 < n_hyp ? h0 : n_hyp - 1), *b = hyp + 4 * (h1 < n_hyp ? h1 : n_hyp - 1);
  const plane_f2 nx = {a[0], b[0]}, ny = {a[1], b[1]}, nz = {a[2], b[2]}, d = {a[3], b[3]};
  int32_t c0 = 0, c1 = 0;
#pragma unroll 4  // (four records' scalar loads in flight ahead of their arithmetic)
  for (int64_t k = k0; k < k1; k++) {
    const float4 p = P[k];  // (wave-uniform: a scalar load)
    const plane_f2 s = ((nx * plane_f2{p.x, p.x} + ny * plane_f2{p.y, p.y}) + nz * plane_f2{p.z, p.z}) + d;
    bool in0 = fabsf(s.x) < max_dist, in1 = fabsf(s.y) < max_dist;
    if (kNormals) {
      const float4 m = N[k];
      const plane_f2 c = (nx * plane_f2{m.x, m.x} + ny * plane_f2{m.y, m.y}) + nz * plane_f2{m.z, m.z};
      in0 = in0 && fabsf(c.x) >= min_normal_cos;
      in1 = in1 && fabsf(c.y) >= min_normal_cos;
    }
    c0 += in0 ? 1 : 0;
    c1 += in1 ? 1 : 0;
  }
  if (ok0 && c0) atomicAdd(&counts[h0], c0);
  if (ok1 && c1) atomicAdd(&counts[h1], c1);
}

__global__ __launch_bounds__(64) void planes_refit_kernel(PlaneState *__restrict__ S, const double *__restrict__ centroid,
                                                          const double *__restrict__ eig, const double *__restrict__ axes,
                                                          PlaneAxis ax) {
  if (threadIdx.x != 0 || !S->found) return;
  float pl[4];
  const double c[3] = {centroid[0], centroid[1], centroid[2]}, a2[3] = {axes[6], axes[7], axes[8]};
  const bool ok = plane_refit(c, a2, eig[0], ax, pl);
  S->refit_ok = ok ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 4; k++) S->rec[1][k] = pl[k];
}

}  // namespace pcgx

using namespace pcgx;

namespace {

pcgx_status planes_check(const char *fn, const pcgx_kdtree *t, const void *samples, int64_t n_hyp, int32_t max_planes,
                         float max_dist, int64_t min_inliers, const float *axis, float min_axis_cos, const void *normals,
                         float min_normal_cos) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  PCGX_TRY(peel_check_counts(fn, n_hyp, "max_planes", max_planes, max_dist, min_inliers));
  PCGX_TRY(peel_check_axis(fn, axis, min_axis_cos));
  if (normals && (!(min_normal_cos >= 0.0f) || !(min_normal_cos <= 1.0f)))
    return fail(PCGX_E_INVALID, "%s: min_normal_cos must be in [0, 1]", fn);
  return peel_check_sizes(fn, t, samples, n_hyp, max_planes);
}

}  // namespace

extern "C" int32_t pcgx_planes_tile(void) { return kPlTile; }

extern "C" pcgx_status pcgx_kdtree_planes_dev(const pcgx_kdtree *t, const uint32_t *d_samples, int64_t n_hyp,
                                              int32_t max_planes, float max_dist, int64_t min_inliers, const float *axis,
                                              float min_axis_cos, const float *d_normals, float min_normal_cos,
                                              int32_t refine, int32_t *d_n_planes, float *d_planes, int32_t *d_sizes,
                                              int32_t *d_refined, int32_t *d_best, int32_t *d_labels, int32_t *d_ids,
                                              int32_t *d_status, int32_t *d_counts, float *d_hyp_planes, void *stream) {
  PCGX_API_LOCK();
  const char *fn = "pcgx_kdtree_planes_dev";
  PCGX_TRY(planes_check(fn, t, d_samples, n_hyp, max_planes, max_dist, min_inliers, axis, min_axis_cos, d_normals,
                        min_normal_cos));
  const int64_t n = t->n;
  if (!d_n_planes || !d_planes || !d_sizes || !d_refined || !d_best || (n > 0 && !d_labels))
    return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  PeelOut o{d_n_planes, d_planes, d_sizes, d_refined, d_best, d_labels, d_ids, d_status, d_counts, d_hyp_planes};
  if (n == 0 || n_hyp == 0) return peel_empty<PlaneModel::kRec>(n, n_hyp * max_planes, max_planes, o, st);
  Arena &ar = ctx().arena;
  PCGX_TRY(ar.begin(st));
  const uint32_t *inv = nullptr;
  PCGX_TRY(range_inverse_map(t, &inv, st));
  const bool with_normals = d_normals != nullptr;
  PeelBuffers<PlaneModel::kRec> b;
  PCGX_TRY(peel_buffers(t, ar, n_hyp, with_normals, refine != 0, &o, &b, st));
  double *gs = nullptr;  // centroid [3], eig [3], axes [9]
  PCGX_TRY(ar.alloc_n(15, &gs));
  const PlaneAxis ax = plane_axis(axis, min_axis_cos);
  const PlaneModel::Test T{max_dist, min_normal_cos};
  // (the records by id, which only the first compaction reads, lie where round 0 writes)
  PCGX_TRY(peel_first<PlaneModel>(t, inv, b, T, d_normals, b.P[1], b.Nr[1], nullptr, o, st));
  int32_t chunk = 0;
  const dim3 count_grid = peel_count_grid("PCGX_PLANES_SPLIT", n_hyp, n, &chunk);
  const unsigned fit_blocks = (unsigned)((n_hyp + 255) / 256);
  const PlaneState *S = b.S;
  return peel_rounds<PlaneModel>(
      b, (int32_t)n, n_hyp, max_planes, min_inliers, refine, T, nullptr, o, st,
      [&](const PeelRound &q) {
        const int32_t *status = q.status;
        const float *hyp = q.hyp;
        hipLaunchKernelGGL(planes_fit_kernel, dim3(fit_blocks), dim3(256), 0, st, S, q.P, d_samples + 3 * n_hyp * q.r, n_hyp,
                           ax, q.status, q.counts, q.hyp);
        if (with_normals)
          hipLaunchKernelGGL(planes_count_kernel<true>, count_grid, dim3(kPlBlock), 0, st, S, q.P, q.N, n_hyp, status, hyp,
                             max_dist, min_normal_cos, chunk, q.counts);
        else
          hipLaunchKernelGGL(planes_count_kernel<false>, count_grid, dim3(kPlBlock), 0, st, S, q.P, q.N, n_hyp, status, hyp,
                             max_dist, min_normal_cos, chunk, q.counts);
      },
      [&](const PeelRound &) -> pcgx_status {
        const Arena::Mark mark = ar.mark();
        PCGX_TRY(group_frames_enqueue(t, b.cand, n, &b.S->cand_size, 1, gs, gs + 3, gs + 6, st));
        ar.rewind(mark);
        const double *g = gs;
        hipLaunchKernelGGL(planes_refit_kernel, dim3(1), dim3(64), 0, st, b.S, g, g + 3, g + 6, ax);
        return PCGX_OK;
      });
}

extern "C" pcgx_status pcgx_kdtree_planes(const pcgx_kdtree *t, const uint32_t *samples, int64_t n_hyp, int32_t max_planes,
                                          float max_dist, int64_t min_inliers, const float *axis, float min_axis_cos,
                                          const float *normals, float min_normal_cos, int32_t refine, int64_t *n_planes,
                                          float *planes, int64_t *sizes, int32_t *refined, int64_t *best, int64_t *labels,
                                          int64_t *ids, int32_t *status, int64_t *counts, float *hyp_planes) {
  PCGX_API_CALL();
  const char *fn = "pcgx_kdtree_planes";
  PCGX_TRY(planes_check(fn, t, samples, n_hyp, max_planes, max_dist, min_inliers, axis, min_axis_cos, normals,
                        min_normal_cos));
  if (!n_planes || !planes || !sizes || !refined || !best || (t->n > 0 && !labels))
    return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  return peel_host<PlaneModel::kRec>(
      t->n, 3, samples, n_hyp, max_planes, normals, n_planes, planes, sizes, refined, best, labels, ids, status, counts,
      hyp_planes, [&](const uint32_t *d_samples, const float *d_normals, const PeelOut &d, hipStream_t st) {
        return pcgx_kdtree_planes_dev(t, d_samples, n_hyp, max_planes, max_dist, min_inliers, axis, min_axis_cos, d_normals,
                                      min_normal_cos, refine, d.n_found, d.recs, d.sizes, d.refined, d.best, d.labels, d.ids,
                                      d.status, d.counts, d.hyp, st);
      });
}
