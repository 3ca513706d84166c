// voxel_cell.h -- the VoxelGrid filter's arithmetic: the grid of a call and the cell of a point, in the reference's
// float32 / int64 arithmetic (pc/filter/voxelgrid/voxelgrid.go:45-79,137-151).  Of HIP it uses the __host__ / __device__
// qualifiers only, which <hip/hip_runtime.h> brings, and nothing of the library: the same text is compiled for the device,
// for the library's host side, and by a plain C++ compiler under its sanitizers, where tests/cpp/host_shim's stand-in
// for that header defines the qualifiers away (tests/cpp/voxel_cell_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace pcgx {

struct VoxelParams {
  float vmin[3];
  float leaf[3];
  int64_t xs, ys;      // strides of the dense index (voxelgrid.go:137,151)
  int64_t n_voxels;    // (xs+1)(ys+1)(zs+1) (voxelgrid.go:138)
  // chunked mode (voxelgrid.go:49-79)
  int32_t chunked;
  float cs[3];         // clamped chunk size in metres
  int64_t nx, ny, n_chunks;
  // chunked mode with (chunk id, cell) fitting 32 bits: ONE sort key = cid * n_voxels + cell
  int32_t combined, pad_;
};

__device__ __forceinline__ void chunk_origin(const VoxelParams &vp, uint32_t cid, float o[3]) {
  // cid2xyz + vMin.Add(cp.ElementMul(chunkSize))  (voxelgrid.go:69-75,109-110)
  // (cid, nx, ny < 2^32, voxel_grid_params: the reference's int arithmetic in 32-bit registers)
  const uint32_t nx = (uint32_t)vp.nx, ny = (uint32_t)vp.ny;
  const uint32_t c2 = cid / nx;
  const uint32_t x = cid - c2 * nx;
  const uint32_t z = c2 / ny;
  const uint32_t y = c2 - z * ny;
  o[0] = vp.vmin[0] + (float)x * vp.cs[0];
  o[1] = vp.vmin[1] + (float)y * vp.cs[1];
  o[2] = vp.vmin[2] + (float)z * vp.cs[2];
}

// (int64_t)q of a float32 quotient that lies in (-1, 2^31): the truncation is 0 for the negative ones, the value fits a
// register -- every point of a cloud whose min / max the grid was made from, NaN and a negative vMin (non-chunked)
// aside.  The general conversion (float -> int64: a dozen instructions) and the 64-bit index arithmetic behind it
// were two thirds of the key kernels' instructions: those kernels were bound by vector issue, not by memory.
__device__ __forceinline__ bool cell_u32(float q, uint32_t &v) {
  const bool ok = q > -1.0f && q < 2147483648.0f;
  v = (uint32_t)(int32_t)(ok ? q : 0.0f);
  return ok;
}

// int(f) of a float32 as the reference's amd64 build computes it (CVTTSS2SQ): truncation, and the "integer indefinite"
// INT64_MIN for a NaN and for |f| >= 2^63.  C++ leaves those casts undefined, and the two sides of this library gave
// different values: x86 the one above, the device 0 for a NaN and a saturated value for the rest -- a valid cell, where
// the Go code's index is out of range.  Every int64 conversion of the grid and of the general cell goes through here,
// so host, device and reference agree by construction.  (cell_u32's lanes never held such a value.)
__host__ __device__ inline int64_t trunc_i64(float f) {
  return (f >= -9223372036854775808.0f && f < 9223372036854775808.0f) ? (int64_t)f : INT64_MIN;
}

// The cell of a point in the reference's arithmetic (float32 subtract and divide, truncation, the xs / ys strides of
// voxelgrid.go:137-151; chunked mode: the chunk first, voxelgrid.go:76-79): the sort key (cell, or chunk id and cell
// in one word), the chunk id and the cell by themselves.  bad: the Go code would panic (index out of range); the
// key is then 0 (an out-of-range chunk) or carries cell 0.  (The general form: any float, 64-bit indices.)
__device__ inline uint32_t voxel_key_xyz_any(const float pt[3], const VoxelParams &vp, uint32_t &cid_out, uint32_t &ka_out, bool &bad) {
  float origin[3] = {vp.vmin[0], vp.vmin[1], vp.vmin[2]};
  uint32_t cid = 0;
  bad = false;
  cid_out = 0;
  ka_out = 0;
  if (vp.chunked) {
    const float q0 = pt[0] - vp.vmin[0], q1 = pt[1] - vp.vmin[1], q2 = pt[2] - vp.vmin[2];
    const int64_t cx = trunc_i64(q0 / vp.cs[0]), cy = trunc_i64(q1 / vp.cs[1]), cz = trunc_i64(q2 / vp.cs[2]);
    // (Go's int arithmetic wraps; C++'s signed overflow is undefined: the products and sums in uint64, the same bits)
    const int64_t c = (int64_t)(((uint64_t)cz * (uint64_t)vp.ny + (uint64_t)cy) * (uint64_t)vp.nx + (uint64_t)cx);
    if (c < 0 || c >= vp.n_chunks) {  // nIndices[cid] would panic
      bad = true;
      return 0u;
    }
    cid = (uint32_t)c;
    chunk_origin(vp, cid, origin);
    cid_out = cid;
  }
  const float p0 = pt[0] - origin[0], p1 = pt[1] - origin[1], p2 = pt[2] - origin[2];
  const int64_t x = trunc_i64(p0 / vp.leaf[0]), y = trunc_i64(p1 / vp.leaf[1]), z = trunc_i64(p2 / vp.leaf[2]);
  const int64_t a = (int64_t)((uint64_t)x + (uint64_t)vp.xs * ((uint64_t)y + (uint64_t)vp.ys * (uint64_t)z));
  uint32_t ka = 0;
  if (a < 0 || a >= vp.n_voxels) bad = true;  // f.voxels[a] would panic
  else ka = (uint32_t)a;
  ka_out = ka;
  return vp.combined ? cid * (uint32_t)vp.n_voxels + ka : ka;
}

// The same result through 32-bit registers where every quotient allows it (cell_u32) and no product leaves 32 bits on
// its way; the general form for the lanes where one does.  xs, ys, nx, ny, n_chunks, n_voxels are all below 2^32
// (voxel_grid_params).
__device__ __forceinline__ uint32_t voxel_key_xyz(const float pt[3], const VoxelParams &vp, uint32_t &cid_out, uint32_t &ka_out,
                                                  bool &bad) {
  float origin[3] = {vp.vmin[0], vp.vmin[1], vp.vmin[2]};
  uint32_t cid = 0;
  bool fast = true;
  if (vp.chunked) {
    const float q0 = pt[0] - vp.vmin[0], q1 = pt[1] - vp.vmin[1], q2 = pt[2] - vp.vmin[2];
    uint32_t cx, cy, cz;
    fast = cell_u32(q0 / vp.cs[0], cx) & cell_u32(q1 / vp.cs[1], cy) & cell_u32(q2 / vp.cs[2], cz);
    // cid2xyz(cid) is (cx, cy, cz) again when cx < nx and cy < ny; cz < 2^31 and ny, nx < 2^32: no product leaves 64 bits
    const uint64_t c = ((uint64_t)cz * (uint32_t)vp.ny + cy) * (uint32_t)vp.nx + cx;
    fast = fast && cx < (uint32_t)vp.nx && cy < (uint32_t)vp.ny && (c >> 32) == 0ull;
    if (fast) {
      if (c >= (uint64_t)vp.n_chunks) {  // nIndices[cid] would panic
        bad = true;
        cid_out = 0;
        ka_out = 0;
        return 0u;
      }
      cid = (uint32_t)c;
      origin[0] = vp.vmin[0] + (float)cx * vp.cs[0];  // vMin.Add(cp.ElementMul(chunkSize))  (voxelgrid.go:69-75,109-110)
      origin[1] = vp.vmin[1] + (float)cy * vp.cs[1];
      origin[2] = vp.vmin[2] + (float)cz * vp.cs[2];
    }
  }
  if (fast) {
    const float p0 = pt[0] - origin[0], p1 = pt[1] - origin[1], p2 = pt[2] - origin[2];
    uint32_t x, y, z;
    fast = cell_u32(p0 / vp.leaf[0], x) & cell_u32(p1 / vp.leaf[1], y) & cell_u32(p2 / vp.leaf[2], z);
    const uint64_t t = (uint64_t)(uint32_t)vp.ys * z + y;                 // < 2^63
    fast = fast && (t >> 32) == 0ull;
    if (fast) {
      const uint64_t a = (uint64_t)(uint32_t)vp.xs * (uint32_t)t + x;     // < 2^64
      bad = a >= (uint64_t)vp.n_voxels;                                    // f.voxels[a] would panic
      const uint32_t ka = bad ? 0u : (uint32_t)a;
      cid_out = cid;
      ka_out = ka;
      return vp.combined ? cid * (uint32_t)vp.n_voxels + ka : ka;
    }
  }
  return voxel_key_xyz_any(pt, vp, cid_out, ka_out, bad);
}

// ---- the grid of a call, from the cloud's min / max (voxelgrid.go:45-62,137-138), in the reference's float32
// arithmetic.  Host and device run the SAME code (the library is built with -ffp-contract=off, float32 divides are
// correctly rounded on both): the bucket path makes its plan on the device, behind the min/max pass, without the host
// in between; the radix path and the error messages use the host's.  Returns 0, or 1 (the chunk grid is not
// addressable) / 2 (the dense grid is empty or exceeds 2^32 cells).
__host__ __device__ inline int voxel_grid_params(const float mm6[6], const float leaf[3], const int32_t chunk[3], VoxelParams &vp) {
  vp = VoxelParams{};
  const float *vmin = mm6, *vmax = mm6 + 3;
  for (int k = 0; k < 3; k++) {
    vp.vmin[k] = vmin[k];
    vp.leaf[k] = leaf[k];
  }
  float size[3];
  if ((int64_t)chunk[0] * chunk[1] * chunk[2] == 0) {
    for (int k = 0; k < 3; k++) size[k] = vmax[k];  // sic (voxelgrid.go:46)
    vp.chunked = 0;
    vp.nx = vp.ny = vp.n_chunks = 1;
  } else {
    float ext[3];
    for (int k = 0; k < 3; k++) {
      ext[k] = vmax[k] - vmin[k];
      vp.cs[k] = leaf[k] * (float)chunk[k];
    }
    for (int k = 0; k < 3; k++)
      if (vp.cs[k] > ext[k] + leaf[k]) vp.cs[k] = ext[k] + leaf[k];
    vp.chunked = 1;
    vp.nx = trunc_i64(ext[0] / vp.cs[0]) + 1;
    vp.ny = trunc_i64(ext[1] / vp.cs[1]) + 1;
    const int64_t nz = trunc_i64(ext[2] / vp.cs[2]) + 1;
    vp.n_chunks = nz;  // (for the message, should the grid not be addressable)
    if (vp.nx <= 0 || vp.ny <= 0 || nz <= 0 || (double)vp.nx * (double)vp.ny * (double)nz >= 4294967296.0) return 1;
    vp.n_chunks = vp.nx * vp.ny * nz;
    for (int k = 0; k < 3; k++) size[k] = vp.cs[k];
  }
  const int64_t xs = trunc_i64(size[0] / leaf[0]), ys = trunc_i64(size[1] / leaf[1]), zs = trunc_i64(size[2] / leaf[2]);
  const double nv = ((double)xs + 1) * ((double)ys + 1) * ((double)zs + 1);
  vp.xs = xs;
  vp.ys = ys;
  vp.n_voxels = zs;  // (for the message)
  if (xs < 0 || ys < 0 || zs < 0 || !(nv >= 1.0) || nv >= 4294967296.0) return 2;
  vp.n_voxels = (xs + 1) * (ys + 1) * (zs + 1);
  return 0;
}

}  // namespace pcgx
