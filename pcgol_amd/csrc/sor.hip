// sor.hip -- statistical outlier removal over an AoS cloud (extension: no reference counterpart; PCL's
// StatisticalOutlierRemoval, Open3D's remove_statistical_outlier).  The contract is include/pcgx.h's pcgx_sor_filter:
//   F = the records whose x, y, z are all finite, m = |F|;
//   d_i = (1/mean_k) sum of sqrt((double)DistSq) over the mean_k points of F \ {i} with the smallest (DistSq, id);
//   mu, sigma (m - 1 in the denominator), T = mu + std_mul sigma, all float64; keep i iff d_i <= T (negative: > T).
// The pipeline, all on the device but the tree build's host part:
//   1. the finite records' xyz, compacted in input order (bucket_grid.h's tile compaction), and their input indices;
//   2. a tree over them (pcgx_kdtree_build: the device build and the grid, by the usual rules);
//   3. knearest.hip in SOR mode, q == NULL, k = mean_k + 1: d_i per tree id (the query's own id left out);
//   4. mu, sigma, T by two reductions of fixed shape (kSorParts partial sums over contiguous chunks, then one
//      workgroup in a fixed tree): the same bits on every call;
//   5. the kept records, byte for byte, compacted in input order (copy_record).
#include <math.h>

#include <memory>

#include "bucket_grid.h"
#include "dbscan.h"

namespace pcgx {

pcgx_status knearest_sor_enqueue(const pcgx_kdtree *t, int32_t mean_k, double *d_mean, hipStream_t st);  // knearest.hip

constexpr int kSorParts = 256;  // partial sums of the statistics (fixed: the summation order is a function of m alone)

__device__ __forceinline__ bool sor_finite(const uint8_t *__restrict__ data, int64_t j, int32_t stride, int32_t off) {
  float v[3];
  __builtin_memcpy(v, data + j * stride + off, 12);
  return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]);
}

__global__ __launch_bounds__(256) void sor_finite_count_kernel(const uint8_t *__restrict__ data, int64_t n, int32_t stride,
                                                               int32_t off, uint32_t *__restrict__ tile_count) {
  tile_flag_count(n, [&](int64_t j) { return sor_finite(data, j, stride, off); }, tile_count);
}
__global__ __launch_bounds__(1024) void sor_scan_kernel(uint32_t *__restrict__ tile_count, int ntiles,
                                                        uint32_t *__restrict__ total) {
  tile_scan(tile_count, ntiles, total);
}
__global__ __launch_bounds__(256) void sor_finite_write_kernel(const uint8_t *__restrict__ data, int64_t n, int32_t stride,
                                                               int32_t off, const uint32_t *__restrict__ tile_offset,
                                                               float *__restrict__ xyz, int64_t *__restrict__ orig) {
  tile_flag_write(n, [&](int64_t j) { return sor_finite(data, j, stride, off); }, tile_offset, [=](uint32_t slot, int64_t j) {
    float v[3];
    __builtin_memcpy(v, data + j * stride + off, 12);
    xyz[3 * (size_t)slot] = v[0];
    xyz[3 * (size_t)slot + 1] = v[1];
    xyz[3 * (size_t)slot + 2] = v[2];
    orig[slot] = j;
  });
}

// mean_dist by input index: NaN for the dropped records (sor_nan_kernel), then d_i for the others (sor_place_kernel)
__global__ __launch_bounds__(256) void sor_nan_kernel(int64_t n, double *__restrict__ md) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) md[j] = __builtin_nan("");
}
__global__ __launch_bounds__(256) void sor_place_kernel(const double *__restrict__ md_c, const int64_t *__restrict__ orig,
                                                        int64_t m, double *__restrict__ md) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < m) md[orig[j]] = md_c[j];
}

// Fixed-shape sum of 256 doubles of a workgroup (thread 0 gets it)
__device__ __forceinline__ double sor_block_sum(double v, double *s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  return s[0];
}

// pass 0: sum d_i; pass 1: sum (d_i - mu)^2.  Workgroup b sums the chunk [b per, (b + 1) per), its thread t the
// elements t, t + 256, ... of it, in order.
template <int kPass>
__global__ __launch_bounds__(256) void sor_partial_kernel(const double *__restrict__ md_c, int64_t m,
                                                          const double *__restrict__ stats, double *__restrict__ part) {
  __shared__ double s[256];
  const int64_t per = (m + kSorParts - 1) / kSorParts;
  const int64_t lo = (int64_t)blockIdx.x * per, hi = min(lo + per, m);
  const double mu = kPass == 1 ? stats[0] : 0.0;
  double acc = 0.0;
  for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
    const double d = md_c[j];
    acc += kPass == 0 ? d : (d - mu) * (d - mu);
  }
  const double tot = sor_block_sum(acc, s);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

template <int kPass>
__global__ __launch_bounds__(256) void sor_final_kernel(const double *__restrict__ part, int64_t m, double std_mul,
                                                        double *__restrict__ stats) {
  __shared__ double s[256];
  const double tot = sor_block_sum(part[threadIdx.x], s);
  if (threadIdx.x != 0) return;
  if (kPass == 0) {
    stats[0] = tot / (double)m;
  } else {
    const double sigma = sqrt(tot / (double)(m - 1));
    stats[1] = sigma;
    stats[2] = stats[0] + std_mul * sigma;
  }
}

__device__ __forceinline__ bool sor_keep(const double *__restrict__ md, int64_t j, double T, int32_t negative) {
  const double d = md[j];  // NaN (a dropped record) is kept in neither mode
  return negative ? d > T : d <= T;
}
__global__ __launch_bounds__(256) void sor_keep_count_kernel(const double *__restrict__ md, int64_t n,
                                                             const double *__restrict__ stats, int32_t negative,
                                                             uint32_t *__restrict__ tile_count) {
  const double T = stats[2];
  tile_flag_count(n, [&](int64_t j) { return sor_keep(md, j, T, negative); }, tile_count);
}
__global__ __launch_bounds__(256) void sor_keep_write_kernel(const double *__restrict__ md, int64_t n,
                                                             const double *__restrict__ stats, int32_t negative,
                                                             const uint32_t *__restrict__ tile_offset,
                                                             const uint8_t *__restrict__ data, int32_t stride,
                                                             uint8_t *__restrict__ out) {
  const double T = stats[2];
  const bool words = ((stride & 3) | ((uintptr_t)data & 3) | ((uintptr_t)out & 3)) == 0;
  tile_flag_write(n, [&](int64_t j) { return sor_keep(md, j, T, negative); }, tile_offset, [=](uint32_t slot, int64_t j) {
    copy_record(data + j * stride, out + (int64_t)slot * stride, stride, words);
  });
}

struct TreeFree {
  void operator()(pcgx_kdtree *t) const { pcgx_kdtree_free(t); }
};

// The whole filter on device records; temporaries from `ka` (begun by the caller), the tree's and the k-NN launch's
// from the context's arena.  d_md: the caller's mean_dist (device, [n]) or nullptr.  Returns with st drained.
pcgx_status sor_run(const uint8_t *d_data, int64_t n, int32_t stride, int32_t off, int32_t mean_k, float std_mul,
                    int32_t negative, uint8_t *d_out, int64_t *out_n, double *d_md, double stats_out[3], hipStream_t st,
                    Arena &ka) {
  const int ntiles = (int)((n + kRunTile - 1) / kRunTile);
  uint32_t *tile_count = nullptr, *d_total = nullptr;
  float *d_xyz = nullptr;
  int64_t *d_orig = nullptr;
  double *d_md_c = nullptr, *d_part = nullptr, *d_stats = nullptr;
  PCGX_TRY(ka.alloc_n((size_t)ntiles, &tile_count));
  PCGX_TRY(ka.alloc_n(2, &d_total));
  PCGX_TRY(ka.alloc_n((size_t)n * 3, &d_xyz));
  PCGX_TRY(ka.alloc_n((size_t)n, &d_orig));
  PCGX_TRY(ka.alloc_n((size_t)n, &d_md_c));
  PCGX_TRY(ka.alloc_n((size_t)kSorParts, &d_part));
  PCGX_TRY(ka.alloc_n(3, &d_stats));
  if (!d_md) PCGX_TRY(ka.alloc_n((size_t)n, &d_md));
  // 1. finite records
  hipLaunchKernelGGL(sor_finite_count_kernel, dim3(ntiles), dim3(256), 0, st, d_data, n, stride, off, tile_count);
  hipLaunchKernelGGL(sor_scan_kernel, dim3(1), dim3(1024), 0, st, tile_count, ntiles, d_total);
  hipLaunchKernelGGL(sor_finite_write_kernel, dim3(ntiles), dim3(256), 0, st, d_data, n, stride, off,
                     (const uint32_t *)tile_count, d_xyz, d_orig);
  PCGX_HIP_TRY(hipGetLastError());
  uint32_t m32 = 0;
  PCGX_HIP_TRY(hipMemcpyAsync(&m32, d_total, 4, hipMemcpyDeviceToHost, st));
  PCGX_HIP_TRY(hipStreamSynchronize(st));
  const int64_t m = m32;
  if (m <= mean_k)
    return fail(PCGX_E_NO_POINT, "pcgx_sor_filter: %lld finite points, mean_k = %d needs more", (long long)m, (int)mean_k);
  // 2. the tree (its host part keeps a copy of the points: they come over once)
  RawVector<float> h_xyz((size_t)m * 3);
  PCGX_TRY(staged_download(h_xyz.data(), d_xyz, (size_t)m * 12, st));
  pcgx_kdtree *raw = nullptr;
  PCGX_TRY(pcgx_kdtree_build(h_xyz.data(), m, 12, 0, &raw));
  std::unique_ptr<pcgx_kdtree, TreeFree> tree(raw);
  // 3. d_i per tree id
  PCGX_TRY(knearest_sor_enqueue(tree.get(), mean_k, d_md_c, st));
  // 4. statistics
  hipLaunchKernelGGL(sor_partial_kernel<0>, dim3(kSorParts), dim3(256), 0, st, (const double *)d_md_c, m,
                     (const double *)d_stats, d_part);
  hipLaunchKernelGGL(sor_final_kernel<0>, dim3(1), dim3(256), 0, st, (const double *)d_part, m, (double)std_mul, d_stats);
  hipLaunchKernelGGL(sor_partial_kernel<1>, dim3(kSorParts), dim3(256), 0, st, (const double *)d_md_c, m,
                     (const double *)d_stats, d_part);
  hipLaunchKernelGGL(sor_final_kernel<1>, dim3(1), dim3(256), 0, st, (const double *)d_part, m, (double)std_mul, d_stats);
  // by input index
  const unsigned nb = (unsigned)((n + 255) / 256), mb = (unsigned)((m + 255) / 256);
  hipLaunchKernelGGL(sor_nan_kernel, dim3(nb), dim3(256), 0, st, n, d_md);
  hipLaunchKernelGGL(sor_place_kernel, dim3(mb), dim3(256), 0, st, (const double *)d_md_c, (const int64_t *)d_orig, m, d_md);
  // 5. the kept records
  hipLaunchKernelGGL(sor_keep_count_kernel, dim3(ntiles), dim3(256), 0, st, (const double *)d_md, n,
                     (const double *)d_stats, negative, tile_count);
  hipLaunchKernelGGL(sor_scan_kernel, dim3(1), dim3(1024), 0, st, tile_count, ntiles, d_total + 1);
  hipLaunchKernelGGL(sor_keep_write_kernel, dim3(ntiles), dim3(256), 0, st, (const double *)d_md, n,
                     (const double *)d_stats, negative, (const uint32_t *)tile_count, d_data, stride, d_out);
  PCGX_HIP_TRY(hipGetLastError());
  uint32_t kept = 0;
  PCGX_HIP_TRY(hipMemcpyAsync(&kept, d_total + 1, 4, hipMemcpyDeviceToHost, st));
  double stats_h[3];
  PCGX_HIP_TRY(hipMemcpyAsync(stats_h, d_stats, sizeof stats_h, hipMemcpyDeviceToHost, st));
  PCGX_HIP_TRY(hipStreamSynchronize(st));  // (the tree is freed below: its kernels must be done)
  *out_n = kept;
  if (stats_out) for (int k = 0; k < 3; k++) stats_out[k] = stats_h[k];
  return PCGX_OK;
}

pcgx_status sor_check(const char *fn, const void *data, int64_t n, int32_t stride, int32_t off, int32_t mean_k,
                      const void *out, const int64_t *out_n) {
  if (!out_n || n < 0 || (n > 0 && (!data || !out))) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (mean_k < 1 || mean_k > 64) return fail(PCGX_E_INVALID, "%s: mean_k = %d outside [1, 64]", fn, (int)mean_k);
  if (stride < 12 || off < 0 || off + 12 > stride)
    return fail(PCGX_E_BAD_FIELD, "%s: stride %d / xyz offset %d do not hold an xyz triple", fn, (int)stride, (int)off);
  if (n == 0) return fail(PCGX_E_NO_POINT, "%s: empty cloud", fn);
  return PCGX_OK;
}

// ------------------------------------------------------------------ radius outlier removal
// pcgx_ror_filter: the same pipeline with a flag in place of the mean distance.  Steps 1, 2 and 5 are the ones above;
// step 3 is density clustering's flag pass (dbscan.hip): the kept points are its core points at min_pts = min_neighbors.
// flag by input index: 0 a dropped record, 1 a point of F with enough neighbours, 2 any other point of F.
__global__ __launch_bounds__(256) void ror_place_kernel(const uint8_t *__restrict__ core, const int64_t *__restrict__ orig,
                                                        int64_t m, uint8_t *__restrict__ flag) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < m) flag[orig[j]] = core[j] ? (uint8_t)1 : (uint8_t)2;
}
__global__ __launch_bounds__(256) void ror_keep_count_kernel(const uint8_t *__restrict__ flag, int64_t n, uint8_t want,
                                                             uint32_t *__restrict__ tile_count) {
  tile_flag_count(n, [&](int64_t j) { return flag[j] == want; }, tile_count);
}
__global__ __launch_bounds__(256) void ror_keep_write_kernel(const uint8_t *__restrict__ flag, int64_t n, uint8_t want,
                                                             const uint32_t *__restrict__ tile_offset,
                                                             const uint8_t *__restrict__ data, int32_t stride,
                                                             uint8_t *__restrict__ out) {
  const bool words = ((stride & 3) | ((uintptr_t)data & 3) | ((uintptr_t)out & 3)) == 0;
  tile_flag_write(n, [&](int64_t j) { return flag[j] == want; }, tile_offset, [=](uint32_t slot, int64_t j) {
    copy_record(data + j * stride, out + (int64_t)slot * stride, stride, words);
  });
}

// The whole filter on device records; temporaries from `ka` (begun by the caller), the tree's and the flag pass's from
// the context's arena.  Returns with st drained.
// flag_pass(tree, d_core): one byte per tree id, nonzero for the points step 5 is to take as 1 (the others as 2).
template <class FlagPass>
pcgx_status flag_filter_run(const char *fn, const uint8_t *d_data, int64_t n, int32_t stride, int32_t off, uint8_t want,
                            FlagPass flag_pass, uint8_t *d_out, int64_t *out_n, hipStream_t st, Arena &ka) {
  const int ntiles = (int)((n + kRunTile - 1) / kRunTile);
  uint32_t *tile_count = nullptr, *d_total = nullptr;
  float *d_xyz = nullptr;
  int64_t *d_orig = nullptr;
  uint8_t *d_core = nullptr, *d_flag = nullptr;
  PCGX_TRY(ka.alloc_n((size_t)ntiles, &tile_count));
  PCGX_TRY(ka.alloc_n(2, &d_total));
  PCGX_TRY(ka.alloc_n((size_t)n * 3, &d_xyz));
  PCGX_TRY(ka.alloc_n((size_t)n, &d_orig));
  PCGX_TRY(ka.alloc_n((size_t)n, &d_core));
  PCGX_TRY(ka.alloc_n((size_t)n, &d_flag));
  // 1. finite records
  hipLaunchKernelGGL(sor_finite_count_kernel, dim3(ntiles), dim3(256), 0, st, d_data, n, stride, off, tile_count);
  hipLaunchKernelGGL(sor_scan_kernel, dim3(1), dim3(1024), 0, st, tile_count, ntiles, d_total);
  hipLaunchKernelGGL(sor_finite_write_kernel, dim3(ntiles), dim3(256), 0, st, d_data, n, stride, off,
                     (const uint32_t *)tile_count, d_xyz, d_orig);
  PCGX_HIP_TRY(hipGetLastError());
  uint32_t m32 = 0;
  PCGX_HIP_TRY(hipMemcpyAsync(&m32, d_total, 4, hipMemcpyDeviceToHost, st));
  PCGX_HIP_TRY(hipStreamSynchronize(st));
  const int64_t m = m32;
  if (m == 0) return fail(PCGX_E_NO_POINT, "%s: no finite point", fn);
  // 2. the tree
  RawVector<float> h_xyz((size_t)m * 3);
  PCGX_TRY(staged_download(h_xyz.data(), d_xyz, (size_t)m * 12, st));
  pcgx_kdtree *raw = nullptr;
  PCGX_TRY(pcgx_kdtree_build(h_xyz.data(), m, 12, 0, &raw));
  std::unique_ptr<pcgx_kdtree, TreeFree> tree(raw);
  // 3. the flag per tree id
  PCGX_TRY(flag_pass(tree.get(), d_core));
  // by input index
  PCGX_HIP_TRY(hipMemsetAsync(d_flag, 0, (size_t)n, st));
  hipLaunchKernelGGL(ror_place_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_core,
                     (const int64_t *)d_orig, m, d_flag);
  // 5. the kept records
  hipLaunchKernelGGL(ror_keep_count_kernel, dim3(ntiles), dim3(256), 0, st, (const uint8_t *)d_flag, n, want, tile_count);
  hipLaunchKernelGGL(sor_scan_kernel, dim3(1), dim3(1024), 0, st, tile_count, ntiles, d_total + 1);
  hipLaunchKernelGGL(ror_keep_write_kernel, dim3(ntiles), dim3(256), 0, st, (const uint8_t *)d_flag, n, want,
                     (const uint32_t *)tile_count, d_data, stride, d_out);
  PCGX_HIP_TRY(hipGetLastError());
  uint32_t kept = 0;
  PCGX_HIP_TRY(hipMemcpyAsync(&kept, d_total + 1, 4, hipMemcpyDeviceToHost, st));
  PCGX_HIP_TRY(hipStreamSynchronize(st));  // (the tree is freed below: its kernels must be done)
  *out_n = kept;
  return PCGX_OK;
}

pcgx_status ror_run(const uint8_t *d_data, int64_t n, int32_t stride, int32_t off, float radius, int32_t min_neighbors,
                    int32_t negative, uint8_t *d_out, int64_t *out_n, hipStream_t st, Arena &ka) {
  return flag_filter_run(
      "pcgx_ror_filter", d_data, n, stride, off, negative ? (uint8_t)2 : (uint8_t)1,
      [&](const pcgx_kdtree *tree, uint8_t *d_core) -> pcgx_status {
        PCGX_TRY(ctx().arena.begin(st));
        return dbscan_core_by_id_enqueue(tree, radius, min_neighbors, d_core, st);
      },
      d_out, out_n, st, ka);
}

// pcgx_thin_filter: the same pipeline once more, step 3 minimum-distance subsampling in hash mode (thin.hip): the kept
// points are its kept set.
pcgx_status thin_kept_by_id(const pcgx_kdtree *t, float radius, uint32_t seed, uint8_t *d_kept, hipStream_t st);

pcgx_status thin_filter_run(const uint8_t *d_data, int64_t n, int32_t stride, int32_t off, float radius, uint32_t seed,
                            uint8_t *d_out, int64_t *out_n, hipStream_t st, Arena &ka) {
  return flag_filter_run(
      "pcgx_thin_filter", d_data, n, stride, off, (uint8_t)1,
      [&](const pcgx_kdtree *tree, uint8_t *d_kept) { return thin_kept_by_id(tree, radius, seed, d_kept, st); }, d_out,
      out_n, st, ka);
}

pcgx_status ror_check(const char *fn, const void *data, int64_t n, int32_t stride, int32_t off, float radius,
                      int32_t min_neighbors, const void *out, const int64_t *out_n) {
  if (!out_n || n < 0 || (n > 0 && (!data || !out))) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!(radius > 0.0f && radius < __builtin_inff())) return fail(PCGX_E_INVALID, "%s: radius must be finite and > 0", fn);
  if (min_neighbors < 1) return fail(PCGX_E_INVALID, "%s: min_neighbors must be >= 1", fn);
  if (stride < 12 || off < 0 || off + 12 > stride)
    return fail(PCGX_E_BAD_FIELD, "%s: stride %d / xyz offset %d do not hold an xyz triple", fn, (int)stride, (int)off);
  if (n == 0) return fail(PCGX_E_NO_POINT, "%s: empty cloud", fn);
  return PCGX_OK;
}

pcgx_status thin_filter_check(const char *fn, const void *data, int64_t n, int32_t stride, int32_t off, float radius,
                              const void *out, const int64_t *out_n) {
  PCGX_TRY(ror_check(fn, data, n, stride, off, radius, 1, out, out_n));
  if (!(radius * radius > 0.0f && radius * radius < __builtin_inff()))
    return fail(PCGX_E_INVALID, "%s: the float32 square of the radius must be finite and > 0", fn);
  return PCGX_OK;
}

}  // namespace pcgx

using namespace pcgx;

extern "C" pcgx_status pcgx_ror_filter_dev(const void *d_data, int64_t n, int32_t stride, int32_t xyz_off, float radius,
                                           int32_t min_neighbors, int32_t negative, void *d_out, int64_t *out_n,
                                           void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(ror_check("pcgx_ror_filter_dev", d_data, n, stride, xyz_off, radius, min_neighbors, d_out, out_n));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  Arena &ka = ctx().host_arena;
  PCGX_TRY(ka.begin(st));
  return ror_run((const uint8_t *)d_data, n, stride, xyz_off, radius, min_neighbors, negative, (uint8_t *)d_out, out_n, st,
                 ka);
}

extern "C" pcgx_status pcgx_ror_filter(const void *data, int64_t n, int32_t stride, int32_t xyz_off, float radius,
                                       int32_t min_neighbors, int32_t negative, void *out_data, int64_t *out_n) {
  PCGX_API_CALL();
  PCGX_TRY(ror_check("pcgx_ror_filter", data, n, stride, xyz_off, radius, min_neighbors, out_data, out_n));
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ka = ctx().host_arena;
  PCGX_TRY(ka.begin(st));
  const size_t bytes = (size_t)n * (size_t)stride;
  uint8_t *d_in = nullptr, *d_out = nullptr;
  PCGX_TRY(ka.alloc_n(bytes, &d_in));
  PCGX_TRY(ka.alloc_n(bytes, &d_out));
  PCGX_TRY(staged_upload(d_in, data, bytes, st));
  int64_t kept = 0;
  PCGX_TRY(ror_run(d_in, n, stride, xyz_off, radius, min_neighbors, negative, d_out, &kept, st, ka));
  if (kept > 0) PCGX_TRY(staged_download(out_data, d_out, (size_t)kept * (size_t)stride, st));
  *out_n = kept;
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_sor_filter_dev(const void *d_data, int64_t n, int32_t stride, int32_t xyz_off, int32_t mean_k,
                                           float std_mul, int32_t negative, void *d_out, int64_t *out_n, double *d_mean_dist,
                                           double stats[3], void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(sor_check("pcgx_sor_filter_dev", d_data, n, stride, xyz_off, mean_k, d_out, out_n));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  Arena &ka = ctx().host_arena;
  PCGX_TRY(ka.begin(st));
  return sor_run((const uint8_t *)d_data, n, stride, xyz_off, mean_k, std_mul, negative, (uint8_t *)d_out, out_n,
                 d_mean_dist, stats, st, ka);
}

extern "C" pcgx_status pcgx_sor_filter(const void *data, int64_t n, int32_t stride, int32_t xyz_off, int32_t mean_k,
                                       float std_mul, int32_t negative, void *out_data, int64_t *out_n, double *mean_dist,
                                       double stats[3]) {
  PCGX_API_CALL();
  PCGX_TRY(sor_check("pcgx_sor_filter", data, n, stride, xyz_off, mean_k, out_data, out_n));
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ka = ctx().host_arena;
  PCGX_TRY(ka.begin(st));
  const size_t bytes = (size_t)n * (size_t)stride;
  uint8_t *d_in = nullptr, *d_out = nullptr;
  double *d_md = nullptr;
  PCGX_TRY(ka.alloc_n(bytes, &d_in));
  PCGX_TRY(ka.alloc_n(bytes, &d_out));
  if (mean_dist) PCGX_TRY(ka.alloc_n((size_t)n, &d_md));
  PCGX_TRY(staged_upload(d_in, data, bytes, st));
  int64_t kept = 0;
  PCGX_TRY(sor_run(d_in, n, stride, xyz_off, mean_k, std_mul, negative, d_out, &kept, d_md, stats, st, ka));
  PCGX_TRY(staged_download(out_data, d_out, (size_t)kept * (size_t)stride, st));
  if (mean_dist) PCGX_TRY(staged_download(mean_dist, d_md, (size_t)n * 8, st));
  *out_n = kept;
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_thin_filter_dev(const void *d_data, int64_t n, int32_t stride, int32_t xyz_off, float radius,
                                            uint32_t seed, void *d_out, int64_t *out_n, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(thin_filter_check("pcgx_thin_filter_dev", d_data, n, stride, xyz_off, radius, d_out, out_n));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  Arena &ka = ctx().host_arena;
  PCGX_TRY(ka.begin(st));
  return thin_filter_run((const uint8_t *)d_data, n, stride, xyz_off, radius, seed, (uint8_t *)d_out, out_n, st, ka);
}

extern "C" pcgx_status pcgx_thin_filter(const void *data, int64_t n, int32_t stride, int32_t xyz_off, float radius,
                                        uint32_t seed, void *out_data, int64_t *out_n) {
  PCGX_API_CALL();
  PCGX_TRY(thin_filter_check("pcgx_thin_filter", data, n, stride, xyz_off, radius, out_data, out_n));
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ka = ctx().host_arena;
  PCGX_TRY(ka.begin(st));
  const size_t bytes = (size_t)n * (size_t)stride;
  uint8_t *d_in = nullptr, *d_out = nullptr;
  PCGX_TRY(ka.alloc_n(bytes, &d_in));
  PCGX_TRY(ka.alloc_n(bytes, &d_out));
  PCGX_TRY(staged_upload(d_in, data, bytes, st));
  int64_t kept = 0;
  PCGX_TRY(thin_filter_run(d_in, n, stride, xyz_off, radius, seed, d_out, &kept, st, ka));
  if (kept > 0) PCGX_TRY(staged_download(out_data, d_out, (size_t)kept * (size_t)stride, st));
  *out_n = kept;
  return PCGX_OK;
}
