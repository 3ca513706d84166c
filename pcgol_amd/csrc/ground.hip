// ground.hip -- ground segmentation: a progressive morphological filter on the caller's grid (extension: no reference
// parity; include/pcgx.h, "ground").  The minimum surface of the live points is opened with squares that grow by the
// caller's schedule; a point is ground while it stays within the schedule's height of every opened surface.  Every step
// is an unsigned min or max over order-preserving keys (group_terms.h) or one float32 subtraction: the result is a
// property of the point set, the same bits on every call, whatever the order anything runs in.
//
//   ground_raster_kernel      a lane per point: its cell (ground_terms.h), its z, window = -1, and an unsigned atomicMin
//                             of the z-key into the cell word (the words start as kGroundEmpty).
//   ground_row_kernel         the morphology, four launches a window (min over rows, min over columns, max over rows,
//                             max over columns: a square is separable and min / max are exact, so this is the
//                             contract's opening).  ONE workgroup holds a whole grid row in LDS (at most 8192 words),
//                             takes the 1-D min or max of half-width h and writes the row as a column of the
//                             transposed surface: the column pass is the same kernel on the transposed surface and
//                             transposes back.  h <= kGrLoopMax: a plain loop over the 2 h + 1 cells.  Above: doubling
//                             in place, M_p[j] = op over [j, j + 2^p) with 2^p <= h + 1 < 2^(p+1), then four reads
//                             a cell: op(M[lo], M[lo + d], M[i], M[i + d]), lo = max(i - h, 0), d = h + 1 - 2^p --
//                             [lo, lo + h] and [i, i + h] -- so the cost grows with log h.
//   ground_classify_kernel    after each window: a point that is still ground and fails the window's test gets window = k.
//   ground_finish_kernel      labels and hag, and per tile of 1024 ids how many are ground and how many are not.
//   ground_scan_kernel        ONE workgroup: the exclusive scans of both counts, sizes[2] and n_groups.
//   ground_scatter_kernel     the two ordered compactions (planes.hip's pattern) and the padding: every slot of ids is
//                             written once.
//   ground_surface_kernel     the cell words as float32, +inf at an empty cell.
// Everything is enqueued at once and nothing is read back.  Integer atomics only.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "ground_terms.h"
#include "group_list.h"

namespace pcgx {

constexpr int kGrBlock = 1024;                 // the row kernel's workgroup: cells of a row one pass handles at once
constexpr int kGrMaxRow = 8192;                // a row in LDS: 32 KB
constexpr int kGrPer = kGrMaxRow / kGrBlock;   // cells of a row a lane holds
constexpr int kGrLoopMax = 64;                 // half-widths up to this take the plain loop (measured: DESIGN 3.24)
constexpr int kGrMaxWin = 64;
constexpr int kGcBlock = 256, kGcIters = 4;
constexpr int kGcTile = kGcBlock * kGcIters;   // ids per workgroup of the compaction
constexpr int kGrOneBlock = 1024;
constexpr int kGrOneWaves = kGrOneBlock / 64;

__global__ __launch_bounds__(256) void ground_raster_kernel(const float4 *__restrict__ nodes, const uint32_t *__restrict__ inv,
                                                            int32_t n, const uint8_t *__restrict__ deleted, GroundGrid g,
                                                            uint32_t *__restrict__ words, int32_t *__restrict__ cell,
                                                            float *__restrict__ zs, int32_t *__restrict__ window) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 nd = node_at(nodes, inv[i]);
  const int32_t c = (deleted && deleted[i]) ? -1 : ground_cell(g, nd.x, nd.y, nd.z);
  cell[i] = c;
  zs[i] = nd.z;
  window[i] = -1;
  if (c >= 0) atomicMin(words + c, ground_key(nd.z));  // (c < nx * ny by ground_cell's test)
}

// in: rows x w, row-major; out: w x rows.  p < 0: the plain loop; else 2^p <= h + 1 < 2^(p+1).
template <bool kMax>
__global__ __launch_bounds__(kGrBlock) void ground_row_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                              int32_t w, int32_t rows, int32_t h, int32_t p) {
  __shared__ uint32_t s[kGrMaxRow];
  const int t = (int)threadIdx.x;
  const int64_t row = blockIdx.x;
  const uint32_t none = kMax ? 0u : kGroundEmpty;
  const uint32_t *src = in + row * w;
#pragma unroll
  for (int j = 0; j < kGrPer; j++) {
    const int i = t + j * kGrBlock;
    if (i < w) s[i] = ground_morph_in<kMax>(src[i]);
  }
  __syncthreads();
  uint32_t r[kGrPer];
  if (p < 0) {
#pragma unroll
    for (int j = 0; j < kGrPer; j++) {
      const int i = t + j * kGrBlock;
      uint32_t acc = none;
      if (i < w) {
        const int lo = i - h > 0 ? i - h : 0, hi = i + h < w - 1 ? i + h : w - 1;
        for (int k = lo; k <= hi; k++) acc = ground_morph_op<kMax>(acc, s[k]);
      }
      r[j] = acc;
    }
  } else {
    for (int step = 0; step < p; step++) {  // (uniform)
      const int off = 1 << step;
#pragma unroll
      for (int j = 0; j < kGrPer; j++) {
        const int i = t + j * kGrBlock;
        uint32_t acc = none;
        if (i < w) acc = ground_morph_op<kMax>(s[i], i + off < w ? s[i + off] : none);
        r[j] = acc;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kGrPer; j++) {
        const int i = t + j * kGrBlock;
        if (i < w) s[i] = r[j];
      }
      __syncthreads();
    }
    const int d = h + 1 - (1 << p);
#pragma unroll
    for (int j = 0; j < kGrPer; j++) {
      const int i = t + j * kGrBlock;
      uint32_t acc = none;
      if (i < w) {
        const int lo = i - h > 0 ? i - h : 0;
        const uint32_t a = ground_morph_op<kMax>(s[lo], lo + d < w ? s[lo + d] : none);
        const uint32_t b = ground_morph_op<kMax>(s[i], i + d < w ? s[i + d] : none);
        acc = ground_morph_op<kMax>(a, b);
      }
      r[j] = acc;
    }
  }
#pragma unroll
  for (int j = 0; j < kGrPer; j++) {
    const int i = t + j * kGrBlock;
    if (i < w) out[(int64_t)i * rows + row] = ground_morph_out<kMax>(r[j]);
  }
}

__global__ __launch_bounds__(256) void ground_classify_kernel(int32_t n, const int32_t *__restrict__ cell,
                                                              const float *__restrict__ zs,
                                                              const uint32_t *__restrict__ words, float height, int32_t k,
                                                              int32_t *__restrict__ window) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t c = cell[i];
  if (c < 0 || window[i] >= 0) return;
  if (!ground_survives(zs[i], words[c], height)) window[i] = k;
}

__global__ __launch_bounds__(kGcBlock) void ground_finish_kernel(int32_t n, const int32_t *__restrict__ cell,
                                                                 const float *__restrict__ zs,
                                                                 const uint32_t *__restrict__ words,
                                                                 const int32_t *__restrict__ window,
                                                                 int32_t *__restrict__ labels, float *__restrict__ hag,
                                                                 int32_t *__restrict__ tile_cnt) {
  __shared__ int32_t s_w[2][kGcBlock / 64];
  const int64_t base = (int64_t)blockIdx.x * kGcTile;
  int32_t c0 = 0, c1 = 0;
#pragma unroll
  for (int j = 0; j < kGcIters; j++) {
    const int64_t i = base + j * kGcBlock + threadIdx.x;
    if (i < n) {
      const int32_t c = cell[i];
      const int32_t lab = c < 0 ? -1 : (window[i] < 0 ? 0 : 1);
      labels[i] = lab;
      if (hag) {
        float v;
        const uint32_t nb = kGroundHagNone;
        __builtin_memcpy(&v, &nb, 4);
        hag[i] = c < 0 ? v : ground_hag(zs[i], words[c]);
      }
      c0 += lab == 0 ? 1 : 0;
      c1 += lab == 1 ? 1 : 0;
    }
  }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    c0 += __shfl_xor(c0, x);
    c1 += __shfl_xor(c1, x);
  }
  if ((threadIdx.x & 63u) == 0u) {
    s_w[0][threadIdx.x >> 6] = c0;
    s_w[1][threadIdx.x >> 6] = c1;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    int32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kGcBlock / 64; w++) sum += s_w[threadIdx.x][w];
    tile_cnt[2 * (int64_t)blockIdx.x + threadIdx.x] = sum;
  }
}

// ONE workgroup: tile_off[2 b + g] = how many ids of group g lie in the tiles before b; sizes and n_groups
__global__ __launch_bounds__(kGrOneBlock) void ground_scan_kernel(int32_t tiles, const int32_t *__restrict__ tile_cnt,
                                                                  int32_t *__restrict__ tile_off, int32_t *__restrict__ sizes,
                                                                  int32_t *__restrict__ n_groups) {
  __shared__ uint32_t s_w[2][kGrOneWaves];
  const int t = (int)threadIdx.x, wave = t >> 6;
  uint32_t carry0 = 0u, carry1 = 0u;
  for (int32_t b = 0; b < tiles; b += kGrOneBlock) {  // uniform
    const int32_t i = b + t;
    const uint32_t v0 = i < tiles ? (uint32_t)tile_cnt[2 * (int64_t)i] : 0u;
    const uint32_t v1 = i < tiles ? (uint32_t)tile_cnt[2 * (int64_t)i + 1] : 0u;
    const uint32_t in0 = wave_incl_scan_u32(v0), in1 = wave_incl_scan_u32(v1);
    if ((t & 63) == 63) {
      s_w[0][wave] = in0;
      s_w[1][wave] = in1;
    }
    __syncthreads();
    uint32_t before0 = 0u, total0 = 0u, before1 = 0u, total1 = 0u;
#pragma unroll
    for (int w = 0; w < kGrOneWaves; w++) {
      const uint32_t a = s_w[0][w], c = s_w[1][w];
      before0 += w < wave ? a : 0u;
      total0 += a;
      before1 += w < wave ? c : 0u;
      total1 += c;
    }
    __syncthreads();
    if (i < tiles) {
      tile_off[2 * (int64_t)i] = (int32_t)(carry0 + before0 + in0 - v0);
      tile_off[2 * (int64_t)i + 1] = (int32_t)(carry1 + before1 + in1 - v1);
    }
    carry0 += total0;
    carry1 += total1;
  }
  if (t != 0) return;
  sizes[0] = (int32_t)carry0;
  sizes[1] = (int32_t)carry1;
  *n_groups = 2;
}

// ids: the ground in ascending order, the rest in ascending order behind it, then one -1 for every id that is not live
__global__ __launch_bounds__(kGcBlock) void ground_scatter_kernel(int32_t n, const int32_t *__restrict__ labels,
                                                                  const int32_t *__restrict__ tile_off,
                                                                  const int32_t *__restrict__ sizes, int32_t *__restrict__ ids) {
  __shared__ uint32_t s_w[2][kGcBlock / 64];
  const int t = (int)threadIdx.x, wave = t >> 6;
  const int64_t base = (int64_t)blockIdx.x * kGcTile;
  const int64_t G = sizes[0], O = sizes[1];
  uint32_t gone0 = (uint32_t)tile_off[2 * (int64_t)blockIdx.x], gone1 = (uint32_t)tile_off[2 * (int64_t)blockIdx.x + 1];
#pragma unroll 1
  for (int j = 0; j < kGcIters; j++) {
    const int64_t i = base + j * kGcBlock + t;
    const int32_t lab = i < n ? labels[i] : -2;
    const uint32_t is0 = lab == 0 ? 1u : 0u, is1 = lab == 1 ? 1u : 0u;
    const uint32_t in0 = wave_incl_scan_u32(is0), in1 = wave_incl_scan_u32(is1);
    if ((t & 63) == 63) {
      s_w[0][wave] = in0;
      s_w[1][wave] = in1;
    }
    __syncthreads();
    uint32_t before0 = 0u, total0 = 0u, before1 = 0u, total1 = 0u;
#pragma unroll
    for (int w = 0; w < kGcBlock / 64; w++) {
      const uint32_t a = s_w[0][w], c = s_w[1][w];
      before0 += w < wave ? a : 0u;
      total0 += a;
      before1 += w < wave ? c : 0u;
      total1 += c;
    }
    __syncthreads();
    if (i < n) {
      const int64_t p0 = (int64_t)(gone0 + before0 + in0 - is0), p1 = (int64_t)(gone1 + before1 + in1 - is1);  // before i
      const int64_t at = lab == 0 ? p0 : (lab == 1 ? G + p1 : G + O + (i - p0 - p1));
      ids[at] = lab < 0 ? -1 : (int32_t)i;  // (at < n: G + O + the ids that are not live = n)
    }
    gone0 += total0;
    gone1 += total1;
  }
}

__global__ __launch_bounds__(256) void ground_surface_kernel(int64_t cells, const uint32_t *__restrict__ words,
                                                             float *__restrict__ surface) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < cells) surface[c] = ground_surface(words[c]);
}

}  // namespace pcgx

using namespace pcgx;

namespace {

bool gr_finite(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return (b & 0x7f800000u) != 0x7f800000u;
}

pcgx_status ground_check(const char *fn, const pcgx_kdtree *t, const float *origin, const int32_t *dims, float cell,
                         int32_t n_win, const int32_t *half, const float *height) {
  if (!t || !origin || !dims) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!gr_finite(cell) || !(cell > 0.0f)) return fail(PCGX_E_INVALID, "%s: cell must be finite and > 0", fn);
  if (!gr_finite(origin[0]) || !gr_finite(origin[1])) return fail(PCGX_E_INVALID, "%s: the origin must be finite", fn);
  if (dims[0] < 1 || dims[0] > kGrMaxRow || dims[1] < 1 || dims[1] > kGrMaxRow)
    return fail(PCGX_E_INVALID, "%s: nx and ny must be in [1, %d]", fn, kGrMaxRow);
  if (n_win < 0 || n_win > kGrMaxWin) return fail(PCGX_E_INVALID, "%s: n_win must be in [0, %d]", fn, kGrMaxWin);
  if (n_win > 0 && (!half || !height)) return fail(PCGX_E_INVALID, "%s: NULL window schedule", fn);
  for (int32_t k = 0; k < n_win; k++) {
    if (half[k] < 1 || half[k] > kGrMaxRow) return fail(PCGX_E_INVALID, "%s: half[%d] must be in [1, %d]", fn, k, kGrMaxRow);
    if (!gr_finite(height[k]) || !(height[k] > 0.0f))
      return fail(PCGX_E_INVALID, "%s: height[%d] must be finite and > 0", fn, k);
  }
  if (t->n > 0x7fffffff) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points", fn);
  return PCGX_OK;
}

// PCGX_GROUND_LOOP_MAX=<h>: the largest half-width that takes the plain loop, forced (measurements).  Read per call.
int32_t ground_loop_max() {
  const char *e = getenv("PCGX_GROUND_LOOP_MAX");
  if (e && *e) {
    const long v = atol(e);
    if (v >= 0) return (int32_t)(v < kGrMaxRow ? v : kGrMaxRow);
  }
  return kGrLoopMax;
}

template <bool kMax>
void ground_pass(const uint32_t *in, uint32_t *out, int32_t w, int32_t rows, int32_t h, int32_t loop_max, hipStream_t st) {
  int32_t p = -1;
  if (h > loop_max) {
    p = 0;
    while ((2 << p) <= h + 1) p++;  // 2^p <= h + 1 < 2^(p+1)
  }
  hipLaunchKernelGGL(ground_row_kernel<kMax>, dim3((unsigned)rows), dim3(kGrBlock), 0, st, in, out, w, rows, h, p);
}

}  // namespace

extern "C" int32_t pcgx_ground_tile(void) { return kGrBlock; }
extern "C" int32_t pcgx_ground_loop_max(void) { return kGrLoopMax; }

extern "C" pcgx_status pcgx_kdtree_ground_dev(const pcgx_kdtree *t, const float *origin, const int32_t *dims, float cell,
                                              int32_t n_win, const int32_t *half, const float *height, int32_t *d_labels,
                                              int32_t *d_sizes, int32_t *d_ids, int32_t *d_n_groups, int32_t *d_window,
                                              float *d_surface, float *d_hag, void *stream) {
  PCGX_API_LOCK();
  const char *fn = "pcgx_kdtree_ground_dev";
  PCGX_TRY(ground_check(fn, t, origin, dims, cell, n_win, half, height));
  const int64_t n = t->n;
  if (!d_sizes || !d_n_groups || (n > 0 && (!d_labels || !d_ids))) return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  Arena &ar = ctx().arena;
  PCGX_TRY(ar.begin(st));
  const GroundGrid g = {origin[0], origin[1], cell, dims[0], dims[1]};
  const int32_t nx = g.nx, ny = g.ny, ni = (int32_t)n;
  const size_t cells = (size_t)nx * (size_t)ny, N = (size_t)n;
  const unsigned tiles = (unsigned)((n + kGcTile - 1) / kGcTile);
  uint32_t *S = nullptr, *T = nullptr;
  int32_t *d_cell = nullptr, *tile_cnt = nullptr, *tile_off = nullptr;
  float *d_z = nullptr;
  uint8_t *d_deleted = nullptr;
  PCGX_TRY(ar.alloc_n(cells, &S));
  if (n_win > 0) PCGX_TRY(ar.alloc_n(cells, &T));
  PCGX_HIP_TRY(hipMemsetAsync(S, 0xff, cells * 4, st));  // kGroundEmpty
  if (n > 0) {
    const uint32_t *inv = nullptr;
    PCGX_TRY(range_inverse_map(t, &inv, st));
    PCGX_TRY(ar.alloc_n(N, &d_cell));
    PCGX_TRY(ar.alloc_n(N, &d_z));
    PCGX_TRY(ar.alloc_n(2 * (size_t)tiles, &tile_cnt));
    PCGX_TRY(ar.alloc_n(2 * (size_t)tiles, &tile_off));
    if (!d_window) PCGX_TRY(ar.alloc_n(N, &d_window));
    {
      pcgx_kdtree *tm = const_cast<pcgx_kdtree *>(t);
      std::lock_guard<std::mutex> lock(tm->mu);
      if (t->n_deleted > 0 && (int64_t)t->deleted.size() == n) {
        PCGX_TRY(ar.alloc_n(N, &d_deleted));
        PCGX_TRY(staged_upload(d_deleted, t->deleted.data(), N, st));
        PCGX_HIP_TRY(hipStreamSynchronize(st));  // (the bytes are the handle's: read before the lock is given up)
      }
    }
    hipLaunchKernelGGL(ground_raster_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t->d_nodes, inv, ni,
                       (const uint8_t *)d_deleted, g, S, d_cell, d_z, d_window);
  }
  const int32_t loop_max = ground_loop_max();
  for (int32_t k = 0; k < n_win; k++) {
    const int32_t h = half[k];
    ground_pass<false>(S, T, nx, ny, h, loop_max, st);  // rows of the surface -> the transposed surface
    ground_pass<false>(T, S, ny, nx, h, loop_max, st);  // its rows are the columns -> back
    ground_pass<true>(S, T, nx, ny, h, loop_max, st);
    ground_pass<true>(T, S, ny, nx, h, loop_max, st);
    if (n > 0)
      hipLaunchKernelGGL(ground_classify_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ni,
                         (const int32_t *)d_cell, (const float *)d_z, (const uint32_t *)S, height[k], k, d_window);
  }
  if (n > 0)
    hipLaunchKernelGGL(ground_finish_kernel, dim3(tiles), dim3(kGcBlock), 0, st, ni, (const int32_t *)d_cell,
                       (const float *)d_z, (const uint32_t *)S, (const int32_t *)d_window, d_labels, d_hag, tile_cnt);
  hipLaunchKernelGGL(ground_scan_kernel, dim3(1), dim3(kGrOneBlock), 0, st, (int32_t)tiles, (const int32_t *)tile_cnt,
                     tile_off, d_sizes, d_n_groups);
  if (n > 0)
    hipLaunchKernelGGL(ground_scatter_kernel, dim3(tiles), dim3(kGcBlock), 0, st, ni, (const int32_t *)d_labels,
                       (const int32_t *)tile_off, (const int32_t *)d_sizes, d_ids);
  if (d_surface)
    hipLaunchKernelGGL(ground_surface_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, (int64_t)cells,
                       (const uint32_t *)S, d_surface);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_kdtree_ground(const pcgx_kdtree *t, const float *origin, const int32_t *dims, float cell,
                                          int32_t n_win, const int32_t *half, const float *height, int64_t *labels,
                                          int64_t *sizes, int64_t *ids, int64_t *n_groups, int32_t *window, float *surface,
                                          float *hag) {
  PCGX_API_CALL();
  const char *fn = "pcgx_kdtree_ground";
  PCGX_TRY(ground_check(fn, t, origin, dims, cell, n_win, half, height));
  const int64_t n = t->n;
  if (!sizes || !n_groups || (n > 0 && (!labels || !ids))) return fail(PCGX_E_INVALID, "%s: NULL output", fn);
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  const size_t N = (size_t)n, cells = (size_t)dims[0] * (size_t)dims[1];
  // one block of int32 words: n_groups, sizes, labels, ids
  const size_t words = 3 + 2 * N;
  int32_t *d_out = nullptr, *d_window = nullptr;
  float *d_surface = nullptr, *d_hag = nullptr;
  PCGX_TRY(ha.alloc_n(words, &d_out));
  if (window && N) PCGX_TRY(ha.alloc_n(N, &d_window));
  if (hag && N) PCGX_TRY(ha.alloc_n(N, &d_hag));
  if (surface) PCGX_TRY(ha.alloc_n(cells, &d_surface));
  int32_t *d_sizes = d_out + 1, *d_labels = d_sizes + 2, *d_ids = d_labels + N;
  PCGX_TRY(pcgx_kdtree_ground_dev(t, origin, dims, cell, n_win, half, height, d_labels, d_sizes, d_ids, d_out, d_window,
                                  d_surface, d_hag, st));
  RawVector<int32_t> r(words);
  PCGX_TRY(staged_download(r.data(), d_out, words * 4, st));
  *n_groups = r[0];
  sizes[0] = r[1];
  sizes[1] = r[2];
  for (size_t i = 0; i < N; i++) labels[i] = r[3 + i];
  for (size_t i = 0; i < N; i++) ids[i] = r[3 + N + i];
  if (window && N) PCGX_TRY(staged_download(window, d_window, N * 4, st));
  if (hag && N) PCGX_TRY(staged_download(hag, d_hag, N * 4, st));
  if (surface) PCGX_TRY(staged_download(surface, d_surface, cells * 4, st));
  return PCGX_OK;
}
