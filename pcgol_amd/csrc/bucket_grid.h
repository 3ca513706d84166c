// bucket_grid.h -- the bucket voxel grid's parameters, its address arithmetic and the device building blocks its
// consumers share (segment.hip: buckets, flood fill; sac.hip: sample consensus plane detection).
//
// Reference: pc/storage/voxelgrid/voxelgrid.go:7-122 (VoxelGrid: [][]int buckets, Addr / Add / Get).
// One copy of VoxelGrid.Addr serves the key kernel, the host entry points and the SAC lattice: the SAC score is a
// count over the voxels Addr() names, so its arithmetic must be the grid's own bit for bit.
#pragma once
#include <stdint.h>

#include <vector>

#include "pcgx_internal.h"

namespace pcgx {

struct GridParams {
  float origin[3];
  float resolution_inv;
  int64_t size[3];
  int64_t len;
};

// VoxelGrid.Addr (voxelgrid.go:64-79): int(pos*resolutionInv + 0.5) per axis, Go's float->int truncation.
// NaN or beyond int64: Go's conversion is implementation defined; such a point is outside.  false: outside the grid.
__host__ __device__ __forceinline__ bool grid_addr(const GridParams &gp, float px, float py, float pz, int64_t *addr,
                                                   int64_t xyz[3]) {
  const float p[3] = {px, py, pz};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float pos = p[k] - gp.origin[k];
    const float f = pos * gp.resolution_inv + 0.5f;
    if (!(f == f) || !(f > -9.0e18f) || !(f < 9.0e18f)) return false;
    const int64_t v = (int64_t)f;
    if (v < 0 || v >= gp.size[k]) return false;
    xyz[k] = v;
  }
  *addr = xyz[0] + (xyz[1] + xyz[2] * gp.size[1]) * gp.size[0];
  return true;
}

__device__ __forceinline__ int64_t lower_bound_u32(const uint32_t *__restrict__ a, int64_t n, uint32_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- order-preserving compaction over tiles of kRunTile elements (one 256-lane block per tile):
// (1) tile_flag_count: flagged elements per tile; (2) tile_scan: exclusive scan of the tile counts by one 1024-lane
// block, total -> *total; (3) tile_flag_write: emit(slot, j) for every flagged j, slots ascending with j.
constexpr int kRunTile = 2048;

template <class Flag>
__device__ __forceinline__ void tile_flag_count(int64_t n, Flag flag, uint32_t *__restrict__ tile_count) {
  __shared__ uint32_t ws[4];
  const int64_t base = (int64_t)blockIdx.x * kRunTile;
  uint32_t c = 0;
  for (int r = 0; r < kRunTile / 256; r++) {
    const int64_t j = base + r * 256 + threadIdx.x;
    if (j < n && flag(j)) c++;
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__device__ __forceinline__ void tile_scan(uint32_t *__restrict__ tile_count, int ntiles, uint32_t *__restrict__ total) {
  __shared__ uint32_t ws[16];
  __shared__ uint32_t carry_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int start = 0; start < ntiles; start += 1024) {
    const int i = start + threadIdx.x;
    const uint32_t v = i < ntiles ? tile_count[i] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < wave; w++) wbase += ws[w];
    const uint32_t carry = carry_s;
    if (i < ntiles) tile_count[i] = carry + wbase + inc - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = carry + wbase + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry_s;
}

template <class Flag, class Emit>
__device__ __forceinline__ void tile_flag_write(int64_t n, Flag flag, const uint32_t *__restrict__ tile_offset, Emit emit) {
  __shared__ uint32_t ws[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * kRunTile;
  uint32_t running = tile_offset[blockIdx.x];
  const uint64_t lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int r = 0; r < kRunTile / 256; r++) {
    const int64_t j = base + r * 256 + threadIdx.x;
    const bool head = j < n && flag(j);
    const uint64_t bal = __ballot(head);
    if (lane == 0) ws[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t wbase = 0, round_total = 0;
    for (int w = 0; w < 4; w++) {
      if (w < wave) wbase += ws[w];
      round_total += ws[w];
    }
    if (head) emit(running + wbase + (uint32_t)__popcll(bal & lt_mask), j);
    running += round_total;
    __syncthreads();
  }
}

// One record of `stride` bytes, byte for byte (VoxelGrid's copy: 4-byte words where stride and both buffers allow)
__device__ __forceinline__ void copy_record(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int32_t stride,
                                            bool words) {
  if (words) {
    for (int b = 0; b < stride; b += 4) *(uint32_t *)(dst + b) = *(const uint32_t *)(src + b);
  } else {
    for (int b = 0; b < stride; b++) dst[b] = src[b];
  }
}

}  // namespace pcgx

struct pcgx_bucket_grid {
  int64_t n = 0;  // points offered (Add(point i, i) for i in [0, n))
  float resolution = 0.0f;
  pcgx::GridParams gp;
  // host copies of the CSR buckets (downloaded once): occupied voxels ascending
  std::vector<uint32_t> cell_addr, cell_start, idx_sorted, point_key;
  std::vector<int32_t> cell_of_addr;  // lazily (segment_bfs, grids up to 2^27 voxels): address -> voxel, -1 empty
  std::vector<uint32_t> cell_comp;  // lazily: smallest voxel address of each voxel's component
  bool have_comp = false;
  int64_t n_in = 0;
};
