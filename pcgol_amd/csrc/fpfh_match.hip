// fpfh_match.hip -- nearest and second nearest row of one FPFH descriptor array in another, and the correspondence
// list made from them (extension: no reference parity; include/pcgx.h, "FPFH matching").
//
// Brute force over all pairs: 33 subtractions, 33 multiplications and 33 additions per pair, float32, in the contract's
// order (fpfh_match_terms.h), so the bits are those of the host's loop.  The matrix cores do not help: their f32 rate
// equals the vector rate on this chip, and |a|^2 + |b|^2 - 2 a.b is another float32 function than the contract's.
//   fpfh_usable_kernel  is a row usable (finite, not all zero)?  One word per row of B (a candidate?) and of A (a query?).
//   fpfh_match_kernel   one wave per workgroup, TWO queries per lane, their 33 + 33 floats in registers as 33 pairs
//                       (constant indices), so that every subtraction, multiplication and addition is one packed
//                       float32 instruction over both queries -- each half rounded on its own, the same bits as two
//                       plain ones.  The candidate row is wave-uniform: the compiler takes it through scalar loads,
//                       33 SGPRs, no LDS.  Candidates in ascending j with a strict <: ties go to the smaller id.  A
//                       candidate whose word says "unusable" is skipped by a scalar branch.  blockIdx.y is the chunk
//                       of B (query waves alone do not fill the chip); a chunk's {id, d1, d2} per query go to memory.
//   fpfh_merge_kernel   one thread per query: its chunks' triples in ascending chunk order -- ascending id -- again
//                       with a strict <; an unusable query is {-1, inf, inf}.  No atomics anywhere.
//   fpfh_corr_kernel    ONE workgroup over all queries, 1024 at a time: ratio test, mutual test, and an exclusive scan
//                       of the kept flags (wave scans by DPP, the waves' totals through LDS) that places the pairs in
//                       ascending query order; then the -1 tail and the count.
// Mutual correspondences are two passes of the match (A in B, B in A): D is bit-symmetric, but a pass that also kept a
// column's best would need a second set of registers or atomics on {D, id} words; not built.
#include <math.h>
#include <stdlib.h>

#include "fpfh_match_terms.h"
#include "pcgx_internal.h"

namespace pcgx {

constexpr int kMatchBlock = 64;                // one wave per workgroup
constexpr int kMatchTile = 2 * kMatchBlock;    // queries per workgroup: lane l has tile * 128 + l and + 64 + l
constexpr int kMatchTargetWaves = 65536;       // the split makes about this many waves: measured, DESIGN.md 3.11
constexpr int kMatchMinChunk = 256;            // ... but leaves a chunk at least this many candidates
constexpr int kMatchMaxSplit = 65535;          // gridDim.y
constexpr int kCorrBlock = 1024;

typedef float match_f2 __attribute__((ext_vector_type(2)));

// 64 rows per wave: their 2112 contiguous floats into LDS by coalesced loads, then one row per lane (a row is 33 words:
// the lanes' rows start in different banks).  One thread per row reading its 132 bytes from memory took 0.5 ms for 10^6
// rows, as long as 3 % of the match it precedes.
__global__ __launch_bounds__(kMatchBlock) void fpfh_usable_kernel(const float *__restrict__ rows, int64_t n,
                                                                  uint32_t *__restrict__ usable) {
  __shared__ float s_rows[kMatchBlock * kMatchLen];
  const int lane = (int)threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kMatchBlock;
  const int cnt = (int)(n - r0 < kMatchBlock ? n - r0 : kMatchBlock);
  const float *src = rows + (size_t)kMatchLen * (size_t)r0;
  for (int e = lane; e < cnt * kMatchLen; e += kMatchBlock) s_rows[e] = src[e];
  __syncthreads();
  if (lane < cnt) usable[r0 + lane] = fpfh_row_usable(s_rows + kMatchLen * lane) ? 1u : 0u;
}

// the candidate at distance D into a query's {d1, d2, id}: strict <, so an equal D leaves the earlier id in place and
// becomes the runner-up (D is never NaN between usable rows; an unusable query's triple is dropped by the merge)
__device__ __forceinline__ void match_take(const float D, const int32_t j, float &d1, float &d2, int32_t &id) {
  d2 = fminf(d2, fmaxf(D, d1));
  const bool c = D < d1;
  id = c ? j : id;
  d1 = c ? D : d1;
}

__global__ __launch_bounds__(kMatchBlock) void fpfh_match_kernel(const float *__restrict__ a, int64_t na,
                                                                 const float *__restrict__ b, int64_t nb,
                                                                 const uint32_t *__restrict__ usable, int64_t chunk,
                                                                 int32_t *__restrict__ p_id, float *__restrict__ p_d1,
                                                                 float *__restrict__ p_d2) {
  const int64_t i0 = (int64_t)blockIdx.x * kMatchTile + threadIdx.x, i1 = i0 + kMatchBlock;
  const float *r0 = a + (size_t)kMatchLen * (size_t)(i0 < na ? i0 : na - 1);
  const float *r1 = a + (size_t)kMatchLen * (size_t)(i1 < na ? i1 : na - 1);
  match_f2 q[kMatchLen];
#pragma unroll
  for (int k = 0; k < kMatchLen; k++) q[k] = match_f2{r0[k], r1[k]};
  const float inf = __builtin_inff();
  float d1x = inf, d1y = inf, d2x = inf, d2y = inf;
  int32_t idx = -1, idy = -1;
  const int64_t j0 = (int64_t)blockIdx.y * chunk;
  const int64_t j1 = j0 + chunk < nb ? j0 + chunk : nb;
  for (int64_t j = j0; j < j1; j++) {
    if (!usable[j]) continue;  // (wave-uniform)
    const float *__restrict__ row = b + (size_t)kMatchLen * (size_t)j;
    match_f2 acc = {0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < kMatchLen; k++) {
      const match_f2 d = q[k] - match_f2{row[k], row[k]};
      acc = acc + d * d;
    }
    match_take(acc.x, (int32_t)j, d1x, d2x, idx);
    match_take(acc.y, (int32_t)j, d1y, d2y, idy);
  }
  const size_t at = (size_t)blockIdx.y * (size_t)na;
  if (i0 < na) {
    p_id[at + i0] = idx;
    p_d1[at + i0] = d1x;
    p_d2[at + i0] = d2x;
  }
  if (i1 < na) {
    p_id[at + i1] = idy;
    p_d1[at + i1] = d1y;
    p_d2[at + i1] = d2y;
  }
}

__global__ __launch_bounds__(256) void fpfh_merge_kernel(const uint32_t *__restrict__ usable_a, int64_t na, int32_t split,
                                                         const int32_t *__restrict__ p_id,
                                                         const float *__restrict__ p_d1,
                                                         const float *__restrict__ p_d2, int32_t *__restrict__ ids,
                                                         float *__restrict__ dist_sq, float *__restrict__ second) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= na) return;
  const float inf = __builtin_inff();
  float d1 = inf, d2 = inf;
  int32_t id = -1;
  if (usable_a[i]) {
    for (int32_t s = 0; s < split; s++) {
      const size_t at = (size_t)s * (size_t)na + (size_t)i;
      const float e1 = p_d1[at];
      if (e1 < d1) {  // the chunk's best wins: the runner-up is the loser or the chunk's own
        d2 = fminf(d1, p_d2[at]);
        d1 = e1;
        id = p_id[at];
      } else {
        d2 = fminf(d2, e1);
      }
    }
  }
  ids[i] = id;
  dist_sq[i] = d1;
  if (second) second[i] = d2;
}

__global__ __launch_bounds__(kCorrBlock) void fpfh_corr_kernel(int64_t na, const int32_t *__restrict__ ids,
                                                               const float *__restrict__ dist_sq,
                                                               const float *__restrict__ second,
                                                               const int32_t *__restrict__ back, float max_ratio_sq,
                                                               int32_t *__restrict__ src, int32_t *__restrict__ dst,
                                                               int32_t *__restrict__ n_pairs) {
  __shared__ uint32_t s_wave[kCorrBlock / 64];
  const int t = (int)threadIdx.x, wave = t >> 6;
  uint32_t base = 0u;  // pairs kept before this round (the same in every thread)
  for (int64_t i0 = 0; i0 < na; i0 += kCorrBlock) {
    const int64_t i = i0 + t;
    int32_t id = -1;
    bool keep = false;
    if (i < na) {
      id = ids[i];
      keep = id >= 0 && dist_sq[i] <= max_ratio_sq * second[i];
      if (keep && back) keep = (int64_t)back[id] == i;
    }
    const uint32_t incl = wave_incl_scan_u32(keep ? 1u : 0u);
    if ((t & 63) == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < kCorrBlock / 64; w++) {
      const uint32_t c = s_wave[w];
      before += w < wave ? c : 0u;
      total += c;
    }
    __syncthreads();
    if (keep) {
      const uint32_t at = base + before + incl - 1u;
      src[at] = (int32_t)i;
      dst[at] = id;
    }
    base += total;
  }
  for (int64_t i = (int64_t)base + t; i < na; i += kCorrBlock) {
    src[i] = -1;
    dst[i] = -1;
  }
  if (t == 0) *n_pairs = (int32_t)base;
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kMatchMaxRows = 0x7fffffff;  // ids are int32 on the device

pcgx_status match_check(const char *fn, const void *a, int64_t na, const void *b, int64_t nb) {
  if (na < 0 || nb < 0) return fail(PCGX_E_INVALID, "%s: negative count", fn);
  if (na > kMatchMaxRows || nb > kMatchMaxRows) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 rows", fn);
  if (na > 0 && !a) return fail(PCGX_E_INVALID, "%s: NULL a", fn);
  if (nb > 0 && !b) return fail(PCGX_E_INVALID, "%s: NULL b", fn);
  return PCGX_OK;
}

pcgx_status ratio_check(const char *fn, float max_ratio_sq) {
  if (!(max_ratio_sq > 0.0f) || !(max_ratio_sq <= 1.0f))
    return fail(PCGX_E_INVALID, "%s: max_ratio_sq must be in (0, 1]", fn);
  return PCGX_OK;
}

// PCGX_MATCH_SPLIT=<n>: the number of chunks of B, forced (tests of the merge, measurements).  Read per call.
int32_t match_split(int64_t na, int64_t nb) {
  const char *e = getenv("PCGX_MATCH_SPLIT");
  if (e && *e) {
    const long v = atol(e);
    if (v > 0) return (int32_t)(v < kMatchMaxSplit ? v : kMatchMaxSplit);
  }
  const int64_t tiles = (na + kMatchTile - 1) / kMatchTile;
  int64_t s = (kMatchTargetWaves + tiles - 1) / tiles;
  const int64_t cap = nb / kMatchMinChunk;
  if (s > cap) s = cap;
  if (s > kMatchMaxSplit) s = kMatchMaxSplit;
  return (int32_t)(s < 1 ? 1 : s);
}

// the match of a's rows in b's, enqueued; temporaries from ctx().arena, which the caller has begun.  na > 0.
pcgx_status match_enqueue(const float *d_a, int64_t na, const float *d_b, int64_t nb, int32_t *d_ids, float *d_dist_sq,
                          float *d_second, hipStream_t st) {
  const int32_t split = match_split(na, nb);
  int64_t chunk = (nb + split - 1) / split;
  if (chunk < 1) chunk = 1;
  Arena &ar = ctx().arena;
  uint32_t *d_usable = nullptr, *d_usable_a = nullptr;
  int32_t *p_id = nullptr;
  float *p_d1 = nullptr, *p_d2 = nullptr;
  PCGX_TRY(ar.alloc_n((size_t)(nb > 0 ? nb : 1), &d_usable));
  PCGX_TRY(ar.alloc_n((size_t)na, &d_usable_a));
  PCGX_TRY(ar.alloc_n((size_t)split * (size_t)na, &p_id));
  PCGX_TRY(ar.alloc_n((size_t)split * (size_t)na, &p_d1));
  PCGX_TRY(ar.alloc_n((size_t)split * (size_t)na, &p_d2));
  if (nb > 0)
    hipLaunchKernelGGL(fpfh_usable_kernel, dim3((unsigned)((nb + kMatchBlock - 1) / kMatchBlock)), dim3(kMatchBlock), 0, st,
                       d_b, nb, d_usable);
  hipLaunchKernelGGL(fpfh_usable_kernel, dim3((unsigned)((na + kMatchBlock - 1) / kMatchBlock)), dim3(kMatchBlock), 0, st,
                     d_a, na, d_usable_a);
  const dim3 grid((unsigned)((na + kMatchTile - 1) / kMatchTile), (unsigned)split);
  hipLaunchKernelGGL(fpfh_match_kernel, grid, dim3(kMatchBlock), 0, st, d_a, na, d_b, nb, (const uint32_t *)d_usable,
                     chunk, p_id, p_d1, p_d2);
  hipLaunchKernelGGL(fpfh_merge_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, st,
                     (const uint32_t *)d_usable_a, na, split, (const int32_t *)p_id, (const float *)p_d1,
                     (const float *)p_d2, d_ids, d_dist_sq, d_second);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

}  // namespace

extern "C" int32_t pcgx_fpfh_match_tile(void) { return kMatchTile; }

extern "C" pcgx_status pcgx_fpfh_match_dev(const float *d_a, int64_t na, const float *d_b, int64_t nb, int32_t *d_ids,
                                           float *d_dist_sq, float *d_second_dist_sq, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(match_check("pcgx_fpfh_match_dev", d_a, na, d_b, nb));
  if (na > 0 && (!d_ids || !d_dist_sq)) return fail(PCGX_E_INVALID, "pcgx_fpfh_match_dev: NULL output");
  if (na == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  PCGX_TRY(ctx().arena.begin(st));
  return match_enqueue(d_a, na, d_b, nb, d_ids, d_dist_sq, d_second_dist_sq, st);
}

extern "C" pcgx_status pcgx_fpfh_correspondences_dev(const float *d_a, int64_t na, const float *d_b, int64_t nb,
                                                     float max_ratio_sq, int32_t mutual, int32_t *d_src_ids,
                                                     int32_t *d_dst_ids, int32_t *d_n_pairs, void *stream) {
  PCGX_API_LOCK();
  const char *fn = "pcgx_fpfh_correspondences_dev";
  PCGX_TRY(match_check(fn, d_a, na, d_b, nb));
  PCGX_TRY(ratio_check(fn, max_ratio_sq));
  if (na > 0 && (!d_src_ids || !d_dst_ids || !d_n_pairs)) return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  if (na == 0) {
    if (d_n_pairs) PCGX_HIP_TRY(hipMemsetAsync(d_n_pairs, 0, sizeof(int32_t), st));
    return PCGX_OK;
  }
  Arena &ar = ctx().arena;
  PCGX_TRY(ar.begin(st));
  int32_t *d_ids = nullptr, *d_back = nullptr;
  float *d_d1 = nullptr, *d_d2 = nullptr, *d_bd1 = nullptr;
  PCGX_TRY(ar.alloc_n((size_t)na, &d_ids));
  PCGX_TRY(ar.alloc_n((size_t)na, &d_d1));
  PCGX_TRY(ar.alloc_n((size_t)na, &d_d2));
  PCGX_TRY(match_enqueue(d_a, na, d_b, nb, d_ids, d_d1, d_d2, st));
  if (mutual && nb > 0) {  // the same rule with the roles swapped: every row of B in A
    PCGX_TRY(ar.alloc_n((size_t)nb, &d_back));
    PCGX_TRY(ar.alloc_n((size_t)nb, &d_bd1));
    PCGX_TRY(match_enqueue(d_b, nb, d_a, na, d_back, d_bd1, nullptr, st));
  }
  hipLaunchKernelGGL(fpfh_corr_kernel, dim3(1), dim3(kCorrBlock), 0, st, na, (const int32_t *)d_ids,
                     (const float *)d_d1, (const float *)d_d2, (const int32_t *)d_back, max_ratio_sq, d_src_ids,
                     d_dst_ids, d_n_pairs);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

namespace {

// a and b on the device, from the calling context's host arena (begun here)
pcgx_status match_stage(const float *a, int64_t na, const float *b, int64_t nb, float **d_a, float **d_b,
                        hipStream_t st) {
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  PCGX_TRY(ha.alloc_n((size_t)na * kMatchLen, d_a));
  PCGX_TRY(staged_upload(*d_a, a, (size_t)na * kMatchLen * 4, st));
  PCGX_TRY(ha.alloc_n((size_t)(nb > 0 ? nb : 1) * kMatchLen, d_b));
  if (nb > 0) PCGX_TRY(staged_upload(*d_b, b, (size_t)nb * kMatchLen * 4, st));
  return PCGX_OK;
}

}  // namespace

extern "C" pcgx_status pcgx_fpfh_match(const float *a, int64_t na, const float *b, int64_t nb, int64_t *ids,
                                       float *dist_sq, float *second_dist_sq) {
  PCGX_API_CALL();
  PCGX_TRY(match_check("pcgx_fpfh_match", a, na, b, nb));
  if (na > 0 && (!ids || !dist_sq)) return fail(PCGX_E_INVALID, "pcgx_fpfh_match: NULL output");
  if (na == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  float *d_a = nullptr, *d_b = nullptr, *d_d1 = nullptr, *d_d2 = nullptr;
  int32_t *d_ids = nullptr;
  PCGX_TRY(match_stage(a, na, b, nb, &d_a, &d_b, st));
  PCGX_TRY(ha.alloc_n((size_t)na, &d_ids));
  PCGX_TRY(ha.alloc_n((size_t)na, &d_d1));
  if (second_dist_sq) PCGX_TRY(ha.alloc_n((size_t)na, &d_d2));
  PCGX_TRY(pcgx_fpfh_match_dev(d_a, na, d_b, nb, d_ids, d_d1, d_d2, st));
  RawVector<int32_t> h_ids((size_t)na);
  PCGX_TRY(staged_download(h_ids.data(), d_ids, (size_t)na * 4, st));
  PCGX_TRY(staged_download(dist_sq, d_d1, (size_t)na * 4, st));
  if (second_dist_sq) PCGX_TRY(staged_download(second_dist_sq, d_d2, (size_t)na * 4, st));
  for (int64_t i = 0; i < na; i++) ids[i] = h_ids[(size_t)i];
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_fpfh_correspondences(const float *a, int64_t na, const float *b, int64_t nb,
                                                 float max_ratio_sq, int32_t mutual, int64_t *src_ids,
                                                 int64_t *dst_ids, int64_t *n_pairs) {
  PCGX_API_CALL();
  const char *fn = "pcgx_fpfh_correspondences";
  PCGX_TRY(match_check(fn, a, na, b, nb));
  PCGX_TRY(ratio_check(fn, max_ratio_sq));
  if (na > 0 && (!src_ids || !dst_ids || !n_pairs)) return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  if (na == 0) {
    if (n_pairs) *n_pairs = 0;
    return PCGX_OK;
  }
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  float *d_a = nullptr, *d_b = nullptr;
  int32_t *d_out = nullptr;  // src [na], dst [na], the count
  PCGX_TRY(match_stage(a, na, b, nb, &d_a, &d_b, st));
  PCGX_TRY(ha.alloc_n((size_t)na * 2 + 1, &d_out));
  PCGX_TRY(pcgx_fpfh_correspondences_dev(d_a, na, d_b, nb, max_ratio_sq, mutual, d_out, d_out + na, d_out + 2 * na,
                                         st));
  RawVector<int32_t> h((size_t)na * 2 + 1);
  PCGX_TRY(staged_download(h.data(), d_out, ((size_t)na * 2 + 1) * 4, st));
  for (int64_t i = 0; i < na; i++) {
    src_ids[i] = h[(size_t)i];
    dst_ids[i] = h[(size_t)(na + i)];
  }
  *n_pairs = h[(size_t)na * 2];
  return PCGX_OK;
}
