// ndt.hip -- the Normal Distributions Transform extension (include/pcgx.h, "Normal Distributions Transform"): a bucket
// voxel grid becomes one Gaussian per voxel (pcgx_ndt_map), and a Fit moves a cloud onto that map by Gauss-Newton on
// Magnusson's score.  NOT in the reference: no parity, checked against tests/ndt_oracle.py.  The arithmetic is
// ndt_terms.h's; this file holds the kernels and the entry points.
//
// Map: ndt_map_kernel, one wave per occupied voxel over the grid's CSR buckets (lanes stride over the voxel's ids in
// bucket order, NormAcc::wave_sum: a fixed order, no atomics), then an order-preserving compaction (bucket_grid.h's
// tile helpers) of the VALID voxels into a sorted address array and one 48-byte record {mean, icov} each.
// Lookup: that sorted array, searched by lower_bound once per x-run of up to three cells (the 27 cells are nine runs,
// the 7 cells one run and four single cells); the x-range of a run is clipped to the row, so a neighbour beyond the
// grid is never the voxel whose address happens to follow.  Chosen over a dense address table because it serves every
// grid the bucket grid allows (up to 2^32 - 2 voxels: a table of that is 16 GiB) from 4 bytes per VALID voxel, which
// stay in L2; the table was not tried.
// Sums: ndt_sums_kernel, a lane per target point, the pose in scalar registers, 30 float64 accumulators per lane reduced
// in the order of icp_gicp_sums_kernel (lanes, waves, workgroup rows), then ndt_final_reduce_kernel, which in a Fit
// also runs the evaluate tail and the Gauss-Newton update in one thread.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bucket_grid.h"
#include "ndt_terms.h"

namespace pcgx {

constexpr int kNdtBlock = 256;
constexpr int kNdtMapBlock = 256;        // four voxels per workgroup
constexpr int kNdtPointsPerLane = 4;     // targets a lane takes before another workgroup is added ...
constexpr int kNdtMaxGrid = 1024;        // ... up to this many workgroups (rows of the partials)

struct NdtMapView {
  const uint32_t *vaddr;  // [nv] addresses of the valid voxels, ascending
  const float4 *rec;      // [3 nv] {mean.xyz, ixx}, {ixy, ixz, iyy, iyz}, {izz, 0, 0, 0}
  int64_t nv;
  GridParams gp;
};

__device__ __forceinline__ double ndt_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;  // lane 0 holds the sum (fixed tree order)
}

// One wave per occupied voxel c: moments over its bucket, the finish by every lane alike, lane 0 writes.
__global__ __launch_bounds__(kNdtMapBlock) void ndt_map_kernel(
    const uint8_t *__restrict__ data, int64_t n, int32_t stride, int32_t off, const uint32_t *__restrict__ cell_addr,
    const uint32_t *__restrict__ cell_start, const uint32_t *__restrict__ idx_sorted, int64_t m, GridParams gp,
    float resolution, int32_t min_points, float min_eigen_ratio, int32_t *__restrict__ count,
    int32_t *__restrict__ valid, float *__restrict__ mean3, float *__restrict__ cov6, float *__restrict__ icov6) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * (kNdtMapBlock / 64) + (threadIdx.x >> 6);
  if (c >= m) return;  // (the whole wave)
  const int64_t addr = (int64_t)cell_addr[c];
  const int64_t v0 = addr % gp.size[0], v1 = (addr / gp.size[0]) % gp.size[1], v2 = addr / (gp.size[0] * gp.size[1]);
  const double ox = ndt_centre(gp.origin[0], v0, resolution), oy = ndt_centre(gp.origin[1], v1, resolution),
               oz = ndt_centre(gp.origin[2], v2, resolution);
  NormAcc acc;
  acc.clear();
  const uint32_t begin = cell_start[c], end = cell_start[c + 1];
  for (uint32_t e = begin + (uint32_t)lane; e < end; e += 64u) {
    const int64_t id = (int64_t)idx_sorted[e];
    if (id >= n) continue;  // (never: the buckets hold ids of the cloud they were built from)
    float p[3];
    __builtin_memcpy(p, data + id * stride + off, 12);
    ndt_acc_add(acc, p[0], p[1], p[2], ox, oy, oz);
  }
  acc.wave_sum();
  NdtVoxel out;
  const bool ok = ndt_voxel_finish(acc, ox, oy, oz, min_points, min_eigen_ratio, out);
  if (lane != 0) return;
  count[c] = acc.n;
  valid[c] = ok ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 3; k++) mean3[3 * c + k] = out.mean[k];
#pragma unroll
  for (int k = 0; k < 6; k++) {
    cov6[6 * c + k] = out.cov6[k];
    icov6[6 * c + k] = out.icov6[k];
  }
}

__global__ __launch_bounds__(256) void ndt_valid_count_kernel(const int32_t *__restrict__ valid, int64_t m,
                                                              uint32_t *__restrict__ tile_count) {
  tile_flag_count(m, [=](int64_t j) { return valid[j] != 0; }, tile_count);
}

__global__ __launch_bounds__(1024) void ndt_valid_scan_kernel(uint32_t *__restrict__ tile_count, int ntiles,
                                                              uint32_t *__restrict__ total) {
  tile_scan(tile_count, ntiles, total);
}

__global__ __launch_bounds__(256) void ndt_valid_write_kernel(const int32_t *__restrict__ valid, int64_t m,
                                                              const uint32_t *__restrict__ tile_offset,
                                                              const uint32_t *__restrict__ cell_addr,
                                                              const float *__restrict__ mean3,
                                                              const float *__restrict__ icov6,
                                                              uint32_t *__restrict__ vaddr, float4 *__restrict__ rec) {
  tile_flag_write(m, [=](int64_t j) { return valid[j] != 0; }, tile_offset, [=](uint32_t slot, int64_t j) {
    vaddr[slot] = cell_addr[j];
    const float *mu = mean3 + 3 * j, *ic = icov6 + 6 * j;
    rec[3 * (int64_t)slot] = make_float4(mu[0], mu[1], mu[2], ic[0]);
    rec[3 * (int64_t)slot + 1] = make_float4(ic[1], ic[2], ic[3], ic[4]);
    rec[3 * (int64_t)slot + 2] = make_float4(ic[5], 0.0f, 0.0f, 0.0f);
  });
}

// Run r of a point's candidate cells: offsets (dy, dz) of its row and the half-width xw of its x-range.
template <int kNb>
__device__ __forceinline__ void ndt_run(const int r, int &dy, int &dz, int &xw) {
  if (kNb == 27) {
    dy = r % 3 - 1;
    dz = r / 3 - 1;
    xw = 1;
  } else if (kNb == 7) {  // the centre run, then y -+ 1, z -+ 1
    dy = r == 1 ? -1 : (r == 2 ? 1 : 0);
    dz = r == 3 ? -1 : (r == 4 ? 1 : 0);
    xw = r == 0 ? 1 : 0;
  } else {
    dy = dz = xw = 0;
  }
}

// The 30 sums of one evaluation.  state != nullptr (a Fit): the pose is state->trans and a finished Fit (done) returns at
// once; else the pose is the kernel argument.  Workgroup b takes targets [b per, (b + 1) per) in a fixed thread
// assignment and leaves its sums in row b of block_partials.
template <int kNb>
__global__ __launch_bounds__(kNdtBlock) void ndt_sums_kernel(const float *__restrict__ target, int64_t nt,
                                                             const IcpState *__restrict__ state, Mat4 pose, NdtMapView mv,
                                                             double half_k2, double two_over_k2,
                                                             double *__restrict__ block_partials) {
  constexpr int NS = (int)P_COUNT;
  constexpr int kRuns = kNb == 27 ? 9 : (kNb == 7 ? 5 : 1);
  __shared__ double s_red[kNdtBlock / 64][NS];
  if (state && state->done) return;  // uniform
  float m[16];
#pragma unroll
  for (int i = 0; i < 16; i++) m[i] = state ? state->trans[i] : pose.m[i];
  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; k++) acc[k] = 0.0;
  const int64_t per = (nt + gridDim.x - 1) / gridDim.x;
  const int64_t r_begin = (int64_t)blockIdx.x * per;
  int64_t r_end = r_begin + per;
  if (r_end > nt) r_end = nt;
  const int64_t sx = mv.gp.size[0], sy = mv.gp.size[1], sz = mv.gp.size[2];
  for (int64_t i = r_begin + threadIdx.x; i < r_end; i += kNdtBlock) {
    float px, py, pz;
    mat4_transform(m, target[3 * i], target[3 * i + 1], target[3 * i + 2], px, py, pz);
    int64_t addr, v[3];
    if (!grid_addr(mv.gp, px, py, pz, &addr, v)) continue;
    for (int r = 0; r < kRuns; r++) {
      int dy, dz, xw;
      ndt_run<kNb>(r, dy, dz, xw);
      const int64_t y = v[1] + dy, z = v[2] + dz;
      if (y < 0 || y >= sy || z < 0 || z >= sz) continue;
      const int64_t x_lo = v[0] - xw < 0 ? 0 : v[0] - xw, x_hi = v[0] + xw >= sx ? sx - 1 : v[0] + xw;
      const int64_t row = (y + z * sy) * sx;
      const uint32_t a_hi = (uint32_t)(row + x_hi);
      for (int64_t j = lower_bound_u32(mv.vaddr, mv.nv, (uint32_t)(row + x_lo)); j < mv.nv && mv.vaddr[j] <= a_hi; j++) {
        const float4 r0 = mv.rec[3 * j], r1 = mv.rec[3 * j + 1], r2 = mv.rec[3 * j + 2];
        const float mean[3] = {r0.x, r0.y, r0.z};
        const float ic[6] = {r0.w, r1.x, r1.y, r1.z, r1.w, r2.x};
        double e, g[6], H[21], w;
        ndt_pair_terms(px, py, pz, mean, ic, half_k2, two_over_k2, e, g, H, w);
        acc[P_VALUE] += e;
#pragma unroll
        for (int a = 0; a < 6; a++) acc[P_G0 + a] += g[a];
#pragma unroll
        for (int a = 0; a < 21; a++) acc[P_H0 + a] += H[a];
        acc[P_WEIGHT] += w;
        acc[P_PAIRS] += 1.0;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; k++) {
    const double s = ndt_wave_sum(acc[k]);
    if (lane == 0) s_red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    double s = 0.0;
    for (int w = 0; w < kNdtBlock / 64; w++) s += s_red[w][threadIdx.x];
    block_partials[(int64_t)blockIdx.x * NS + threadIdx.x] = s;
  }
}

// The evaluate tail (finish_evaluate_plane behind the min_pairs test) + the Gauss-Newton update + the loop's
// bookkeeping, as the plane session has them; one thread.
__device__ __forceinline__ void ndt_update_step(IcpState *__restrict__ state, const double *__restrict__ sums30,
                                                const IcpKernelParams &kp) {
  state->num_iteration += 1;
  const int64_t npairs = (int64_t)sums30[P_PAIRS];
  if (npairs < (int64_t)kp.min_pairs) {
    state->ev.num_pairs = npairs;
    state->status = PCGX_E_NOT_ENOUGH_PAIRS;
    state->done = 1;
    return;
  }
  EvaluatedPlane ev;
  finish_evaluate_plane(sums30, ev);
  state->ev.value = ev.value;
  for (int i = 0; i < 6; i++) state->ev.gradient[i] = ev.gradient[i];
  state->ev.dist_rms = 0.0f;
  state->ev.num_pairs = ev.num_pairs;
  for (int i = 0; i < 36; i++) state->hessian[i] = ev.hessian[i];
  Mat4 t;
  for (int i = 0; i < 16; i++) t.m[i] = state->trans[i];
  int32_t it = state->iter;
  const int rc = gauss_newton_update(kp.gn, it, ev, t);
  if (rc < 0) {
    state->status = PCGX_E_SINGULAR;
    state->done = 1;
    return;
  }
  for (int i = 0; i < 16; i++) state->trans[i] = t.m[i];
  state->iter = it;
  if (rc > 0) state->done = 1;
}

// The workgroups' rows summed in a fixed order -> sums (wave w owns components w, w + waves, ...); in a Fit (state !=
// nullptr) thread 0 then runs the update.
__global__ __launch_bounds__(1024) void ndt_final_reduce_kernel(const double *__restrict__ block_partials, int nblocks,
                                                                IcpState *__restrict__ state, double *__restrict__ sums,
                                                                IcpKernelParams kp) {
  constexpr int NS = (int)P_COUNT;
  __shared__ double s_sums[NS];
  if (state && state->done) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, waves = blockDim.x >> 6;
  for (int k = wave; k < NS; k += waves) {
    double v = 0.0;
    for (int b = lane; b < nblocks; b += 64) v += block_partials[(int64_t)b * NS + k];
    v = ndt_wave_sum(v);
    if (lane == 0) {
      sums[k] = v;
      s_sums[k] = v;
    }
  }
  if (state) {
    __syncthreads();
    if (threadIdx.x == 0) ndt_update_step(state, s_sums, kp);
  }
}

}  // namespace pcgx

using namespace pcgx;

struct pcgx_ndt_map {
  GridParams gp;
  float resolution = 0.0f;
  int64_t m = 0;   // occupied voxels
  int64_t nv = 0;  // ... of them valid
  uint32_t *d_vaddr = nullptr;  // library-owned
  float4 *d_rec = nullptr;
  // the per-voxel read-out (pcgx_ndt_map_cells), downloaded once
  std::vector<uint32_t> addr;
  std::vector<int32_t> count, valid;
  std::vector<float> mean3, cov6, icov6;
};

static void ndt_map_release(pcgx_ndt_map *m) {
  if (!m) return;
  dev_cache_free(m->d_vaddr);
  dev_cache_free(m->d_rec);
  delete m;
}

extern "C" pcgx_status pcgx_ndt_map_create(const pcgx_bucket_grid *g, const void *data, int64_t n, int32_t stride,
                                           int32_t xyz_off, int32_t on_device, int32_t min_points, float min_eigen_ratio,
                                           pcgx_ndt_map **out) {
  PCGX_API_LOCK();
  if (!out) return fail(PCGX_E_INVALID, "pcgx_ndt_map_create: out is NULL");
  *out = nullptr;
  if (!g || n < 0 || (n > 0 && !data)) return fail(PCGX_E_INVALID, "pcgx_ndt_map_create: bad argument");
  if (n != g->n) return fail(PCGX_E_INVALID, "pcgx_ndt_map_create: %lld points, the grid was built from %lld", (long long)n, (long long)g->n);
  if (!(min_eigen_ratio > 0.0f && min_eigen_ratio <= 1.0f))
    return fail(PCGX_E_INVALID, "pcgx_ndt_map_create: min_eigen_ratio must be in (0, 1]");
  if (n > 0 && (stride < 12 || xyz_off < 0 || xyz_off + 12 > stride))
    return fail(PCGX_E_BAD_FIELD, "pcgx_ndt_map_create: stride %d / xyz offset %d do not hold an xyz triple", stride, xyz_off);
  pcgx_ndt_map *map = new pcgx_ndt_map();
  map->gp = g->gp;
  map->resolution = g->resolution;
  map->m = (int64_t)g->cell_addr.size();
  if (map->m == 0) {  // an empty grid: a map with no voxels
    *out = map;
    return PCGX_OK;
  }
  pcgx_status rc = ensure_init();
  if (rc != PCGX_OK) {
    delete map;
    return rc;
  }
  hipStream_t st = ctx().stream;
  Arena &ar = ctx().arena;
  const int64_t m = map->m, n_in = g->n_in;
  const int ntiles = (int)((m + kRunTile - 1) / kRunTile);
  auto body = [&]() -> pcgx_status {
    PCGX_HIP_TRY(dev_cache_alloc((void **)&map->d_vaddr, (size_t)m * 4));
    PCGX_HIP_TRY(dev_cache_alloc((void **)&map->d_rec, (size_t)m * 3 * sizeof(float4)));
    PCGX_TRY(ar.begin(st));
    uint32_t *d_addr = nullptr, *d_start = nullptr, *d_idx = nullptr, *d_tiles = nullptr, *d_total = nullptr;
    int32_t *d_count = nullptr, *d_valid = nullptr;
    float *d_mean = nullptr, *d_cov = nullptr, *d_icov = nullptr;
    PCGX_TRY(ar.alloc_n((size_t)m, &d_addr));
    PCGX_TRY(ar.alloc_n((size_t)m + 1, &d_start));
    PCGX_TRY(ar.alloc_n((size_t)n_in, &d_idx));
    PCGX_TRY(ar.alloc_n((size_t)ntiles, &d_tiles));
    PCGX_TRY(ar.alloc_n(1, &d_total));
    PCGX_TRY(ar.alloc_n((size_t)m, &d_count));
    PCGX_TRY(ar.alloc_n((size_t)m, &d_valid));
    PCGX_TRY(ar.alloc_n((size_t)m * 3, &d_mean));
    PCGX_TRY(ar.alloc_n((size_t)m * 6, &d_cov));
    PCGX_TRY(ar.alloc_n((size_t)m * 6, &d_icov));
    const uint8_t *src = (const uint8_t *)data;
    if (!on_device) {
      uint8_t *d_raw = nullptr;
      PCGX_TRY(ar.alloc_n((size_t)n * stride, &d_raw));
      PCGX_HIP_TRY(hipMemcpyAsync(d_raw, data, (size_t)n * stride, hipMemcpyHostToDevice, st));
      src = d_raw;
    }
    PCGX_HIP_TRY(hipMemcpyAsync(d_addr, g->cell_addr.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
    PCGX_HIP_TRY(hipMemcpyAsync(d_start, g->cell_start.data(), (size_t)(m + 1) * 4, hipMemcpyHostToDevice, st));
    PCGX_HIP_TRY(hipMemcpyAsync(d_idx, g->idx_sorted.data(), (size_t)n_in * 4, hipMemcpyHostToDevice, st));
    const unsigned map_grid = (unsigned)((m + kNdtMapBlock / 64 - 1) / (kNdtMapBlock / 64));
    hipLaunchKernelGGL(ndt_map_kernel, dim3(map_grid), dim3(kNdtMapBlock), 0, st, src, n, stride, xyz_off, d_addr, d_start,
                       d_idx, m, map->gp, map->resolution, min_points, min_eigen_ratio, d_count, d_valid, d_mean, d_cov,
                       d_icov);
    hipLaunchKernelGGL(ndt_valid_count_kernel, dim3(ntiles), dim3(256), 0, st, d_valid, m, d_tiles);
    hipLaunchKernelGGL(ndt_valid_scan_kernel, dim3(1), dim3(1024), 0, st, d_tiles, ntiles, d_total);
    hipLaunchKernelGGL(ndt_valid_write_kernel, dim3(ntiles), dim3(256), 0, st, d_valid, m, d_tiles, d_addr, d_mean, d_icov,
                       map->d_vaddr, map->d_rec);
    PCGX_HIP_TRY(hipGetLastError());
    map->addr = g->cell_addr;
    map->count.resize((size_t)m);
    map->valid.resize((size_t)m);
    map->mean3.resize((size_t)m * 3);
    map->cov6.resize((size_t)m * 6);
    map->icov6.resize((size_t)m * 6);
    uint32_t total = 0;
    PCGX_HIP_TRY(hipMemcpyAsync(map->count.data(), d_count, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    PCGX_HIP_TRY(hipMemcpyAsync(map->valid.data(), d_valid, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    PCGX_HIP_TRY(hipMemcpyAsync(map->mean3.data(), d_mean, (size_t)m * 12, hipMemcpyDeviceToHost, st));
    PCGX_HIP_TRY(hipMemcpyAsync(map->cov6.data(), d_cov, (size_t)m * 24, hipMemcpyDeviceToHost, st));
    PCGX_HIP_TRY(hipMemcpyAsync(map->icov6.data(), d_icov, (size_t)m * 24, hipMemcpyDeviceToHost, st));
    PCGX_HIP_TRY(hipMemcpyAsync(&total, d_total, 4, hipMemcpyDeviceToHost, st));
    // the grid and the caller's buffers (host or device) are free to change once this returns
    PCGX_HIP_TRY(hipStreamSynchronize(st));
    map->nv = (int64_t)total;
    return PCGX_OK;
  };
  rc = body();
  if (rc != PCGX_OK) {
    (void)hipStreamSynchronize(st);
    ndt_map_release(map);
    return rc;
  }
  *out = map;
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_ndt_map_free(pcgx_ndt_map *m) {
  PCGX_API_LOCK();
  if (m && m->d_vaddr) dev_cache_quiesce();  // (a _dev evaluation may still be in flight on the caller's stream)
  ndt_map_release(m);
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_ndt_map_counts(const pcgx_ndt_map *m, int64_t *n_occupied, int64_t *n_valid) {
  PCGX_API_LOCK();
  if (!m) return fail(PCGX_E_INVALID, "pcgx_ndt_map_counts: NULL map");
  if (n_occupied) *n_occupied = m->m;
  if (n_valid) *n_valid = m->nv;
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_ndt_map_cells(const pcgx_ndt_map *m, int64_t *addr, int32_t *count, int32_t *valid,
                                          float *mean3, float *cov6, float *icov6) {
  PCGX_API_LOCK();
  if (!m) return fail(PCGX_E_INVALID, "pcgx_ndt_map_cells: NULL map");
  const size_t k = (size_t)m->m;
  if (k == 0) return PCGX_OK;
  if (addr)
    for (size_t c = 0; c < k; c++) addr[c] = (int64_t)m->addr[c];
  if (count) memcpy(count, m->count.data(), k * 4);
  if (valid) memcpy(valid, m->valid.data(), k * 4);
  if (mean3) memcpy(mean3, m->mean3.data(), k * 12);
  if (cov6) memcpy(cov6, m->cov6.data(), k * 24);
  if (icov6) memcpy(icov6, m->icov6.data(), k * 24);
  return PCGX_OK;
}

namespace {

struct NdtConstants {
  double half_k2, two_over_k2;
};

pcgx_status ndt_check(const char *fn, const pcgx_ndt_map *m, const float *target, int64_t nt, int32_t neighbors,
                      float outlier_ratio, NdtConstants *k) {
  if (!m || nt < 0 || (nt > 0 && !target)) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (neighbors != 1 && neighbors != 7 && neighbors != 27) return fail(PCGX_E_INVALID, "%s: neighbors must be 1, 7 or 27", fn);
  double k2 = 0.0;
  if (!ndt_k2(outlier_ratio, m->resolution, &k2))
    return fail(PCGX_E_INVALID, "%s: outlier_ratio %g at resolution %g gives no finite k2 > 0", fn, (double)outlier_ratio,
                (double)m->resolution);
  k->half_k2 = 0.5 * k2;
  k->two_over_k2 = 2.0 / k2;
  return PCGX_OK;
}

int ndt_grid(int64_t nt) {
  const int64_t per = (int64_t)kNdtBlock * kNdtPointsPerLane;
  return (int)std::min<int64_t>(kNdtMaxGrid, std::max<int64_t>(1, (nt + per - 1) / per));
}

NdtMapView ndt_view(const pcgx_ndt_map *m) {
  NdtMapView v;
  v.vaddr = m->d_vaddr;
  v.rec = m->d_rec;
  v.nv = m->nv;
  v.gp = m->gp;
  return v;
}

// One evaluation: the sums kernel and the final reduce behind it (with the update when state != nullptr).
pcgx_status ndt_enqueue(const pcgx_ndt_map *m, const float *d_target, int64_t nt, IcpState *d_state, const Mat4 &pose,
                        int32_t neighbors, const NdtConstants &k, const IcpKernelParams &kp, double *d_partials,
                        double *d_sums, hipStream_t st) {
  const dim3 grid((unsigned)ndt_grid(nt)), block(kNdtBlock);
  const NdtMapView mv = ndt_view(m);
  if (neighbors == 27)
    hipLaunchKernelGGL(ndt_sums_kernel<27>, grid, block, 0, st, d_target, nt, d_state, pose, mv, k.half_k2, k.two_over_k2,
                       d_partials);
  else if (neighbors == 7)
    hipLaunchKernelGGL(ndt_sums_kernel<7>, grid, block, 0, st, d_target, nt, d_state, pose, mv, k.half_k2, k.two_over_k2,
                       d_partials);
  else
    hipLaunchKernelGGL(ndt_sums_kernel<1>, grid, block, 0, st, d_target, nt, d_state, pose, mv, k.half_k2, k.two_over_k2,
                       d_partials);
  hipLaunchKernelGGL(ndt_final_reduce_kernel, dim3(1), dim3(1024), 0, st, d_partials, (int)grid.x, d_state, d_sums, kp);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

Mat4 pose_or_identity(const float *trans16) {
  Mat4 p = mat4_translate(0.0f, 0.0f, 0.0f);
  if (trans16) memcpy(p.m, trans16, sizeof p.m);
  return p;
}

}  // namespace

extern "C" pcgx_status pcgx_ndt_evaluate_dev(const pcgx_ndt_map *m, const float *d_target, int64_t nt,
                                             const float trans16[16], int32_t neighbors, float outlier_ratio,
                                             double *d_sums30, void *stream) {
  PCGX_API_LOCK();
  NdtConstants k;
  PCGX_TRY(ndt_check("pcgx_ndt_evaluate_dev", m, d_target, nt, neighbors, outlier_ratio, &k));
  if (!d_sums30) return fail(PCGX_E_INVALID, "pcgx_ndt_evaluate_dev: NULL sums");
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  Arena &ar = ctx().arena;
  PCGX_TRY(ar.begin(st));
  double *d_partials = nullptr;
  PCGX_TRY(ar.alloc_n((size_t)ndt_grid(nt) * P_COUNT, &d_partials));
  IcpKernelParams kp;
  memset(&kp, 0, sizeof kp);
  return ndt_enqueue(m, d_target, nt, nullptr, pose_or_identity(trans16), neighbors, k, kp, d_partials, d_sums30, st);
}

extern "C" pcgx_status pcgx_ndt_evaluate(const pcgx_ndt_map *m, const float *target, int64_t nt, const float trans16[16],
                                         int32_t neighbors, float outlier_ratio, double sums30[30]) {
  PCGX_API_CALL();
  NdtConstants k;
  PCGX_TRY(ndt_check("pcgx_ndt_evaluate", m, target, nt, neighbors, outlier_ratio, &k));
  if (!sums30) return fail(PCGX_E_INVALID, "pcgx_ndt_evaluate: NULL sums");
  if (nt == 0) {
    for (int i = 0; i < (int)P_COUNT; i++) sums30[i] = 0.0;
    return PCGX_OK;
  }
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_t = nullptr;
  double *d_s = nullptr;
  PCGX_TRY(ha.alloc_n((size_t)nt * 3, &d_t));
  PCGX_TRY(ha.alloc_n((size_t)P_COUNT, &d_s));
  PCGX_TRY(staged_upload(d_t, target, (size_t)nt * 12, st));
  PCGX_TRY(pcgx_ndt_evaluate_dev(m, d_t, nt, trans16, neighbors, outlier_ratio, d_s, st));
  return staged_download(sums30, d_s, sizeof(double) * P_COUNT, st);
}

extern "C" pcgx_status pcgx_ndt_fit(const pcgx_ndt_map *m, const float *target, int64_t nt, int32_t on_device,
                                    const pcgx_icp_params *params, float damping, int32_t neighbors, float outlier_ratio,
                                    const float init16[16], float trans16[16], pcgx_icp_stat *stat, float hessian36[36]) {
  PCGX_API_CALL();
  NdtConstants k;
  PCGX_TRY(ndt_check("pcgx_ndt_fit", m, target, nt, neighbors, outlier_ratio, &k));
  if (!params || !trans16) return fail(PCGX_E_INVALID, "pcgx_ndt_fit: NULL argument");
  if (params->max_iteration < 0 || params->min_pairs < 0) return fail(PCGX_E_INVALID, "pcgx_ndt_fit: negative count");
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena, &ar = ctx().arena;
  IcpKernelParams kp;
  memset(&kp, 0, sizeof kp);
  kp.min_pairs = params->min_pairs == 0 ? 6 : params->min_pairs;
  kp.gn = resolve_gauss_newton(params->threshold, damping, params->max_iteration);
  IcpState h;
  memset(&h, 0, sizeof h);
  const Mat4 init = pose_or_identity(init16);
  memcpy(h.trans, init.m, sizeof h.trans);
  PCGX_TRY(ha.begin(st));
  const float *d_t = target;
  if (!on_device && nt > 0) {
    float *up = nullptr;
    PCGX_TRY(ha.alloc_n((size_t)nt * 3, &up));
    PCGX_TRY(staged_upload(up, target, (size_t)nt * 12, st));
    d_t = up;
  }
  PCGX_TRY(ar.begin(st));
  IcpState *d_state = nullptr;
  double *d_partials = nullptr, *d_sums = nullptr;
  PCGX_TRY(ar.alloc_n(1, &d_state));
  PCGX_TRY(ar.alloc_n((size_t)ndt_grid(nt) * P_COUNT, &d_partials));
  PCGX_TRY(ar.alloc_n((size_t)P_COUNT, &d_sums));
  PCGX_HIP_TRY(hipMemcpyAsync(d_state, &h, sizeof h, hipMemcpyHostToDevice, st));
  // the whole loop is enqueued; an iteration behind the one that set `done` returns at once
  for (int it = 0; it < kp.gn.max_iteration; it++)
    PCGX_TRY(ndt_enqueue(m, d_t, nt, d_state, init, neighbors, k, kp, d_partials, d_sums, st));
  PCGX_HIP_TRY(hipMemcpyAsync(&h, d_state, sizeof h, hipMemcpyDeviceToHost, st));  // the one read-back
  PCGX_HIP_TRY(hipStreamSynchronize(st));
  memcpy(trans16, h.trans, sizeof h.trans);
  if (stat) {
    stat->evaluated.value = h.ev.value;
    memcpy(stat->evaluated.gradient, h.ev.gradient, sizeof h.ev.gradient);
    stat->evaluated.dist_rms = 0.0f;
    stat->evaluated.num_pairs = h.ev.num_pairs;
    stat->num_iteration = h.num_iteration;
  }
  if (hessian36) memcpy(hessian36, h.hessian, sizeof h.hessian);
  if (h.status == PCGX_E_NOT_ENOUGH_PAIRS)
    return fail(PCGX_E_NOT_ENOUGH_PAIRS, "not enough (point, voxel) pairs (%lld < %d) at iteration %d",
                (long long)h.ev.num_pairs, kp.min_pairs, h.num_iteration);
  if (h.status == PCGX_E_SINGULAR)
    return fail(PCGX_E_SINGULAR, "normal equations are not positive definite at iteration %d", h.num_iteration);
  return PCGX_OK;
}
