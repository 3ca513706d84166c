// ground_terms.h -- the decisions of ground segmentation, shared by the device kernels (ground.hip) and the host test
// (tests/cpp/ground_terms_host.cpp over the shim tests/cpp/host_shim): one expression, compiled by both.
// NOT in the reference: no parity, checked against the NumPy oracle's restatement (tests/ground_oracle.py).
//
// Contract (include/pcgx.h, "ground").  All float32, each operation rounded once.
//   cell      fx = floorf((x - ox) / cell), fy = floorf((y - oy) / cell)
//   live      x, y, z finite, 0 <= fx < nx and 0 <= fy < ny compared as floats; then c = (int)fy * nx + (int)fx
//   key       group_terms.h's order-preserving key of z: the minimum surface is an unsigned min over keys
//   empty     a cell word in memory is kGroundEmpty; an erosion reads it as it is (above every key), a dilation reads
//             it as 0 (below every key) and writes 0 back as kGroundEmpty
//   ground    a live point survives a window iff z - S[c] < height, one subtraction, strict
#pragma once
#include "group_terms.h"

namespace pcgx {

constexpr uint32_t kGroundEmpty = 0xffffffffu;   // no finite z has this key (it is a NaN's), nor the key 0
constexpr uint32_t kGroundHagNone = 0x7fc00000u;  // hag of a point that is not live

struct GroundGrid {
  float ox, oy, cell;
  int32_t nx, ny;
};

// the cell of a point, or -1 where the point is not live (a deleted point is the caller's to leave out)
__device__ __forceinline__ int32_t ground_cell(const GroundGrid &g, const float x, const float y, const float z) {
  if (!group_point_ok(x, y, z)) return -1;
  const float fx = floorf((x - g.ox) / g.cell), fy = floorf((y - g.oy) / g.cell);
  if (!(fx >= 0.0f && fx < (float)g.nx && fy >= 0.0f && fy < (float)g.ny)) return -1;
  return (int32_t)fy * g.nx + (int32_t)fx;
}

__device__ __forceinline__ uint32_t ground_key(const float z) { return group_key_f32(z); }
// a cell word as the surface output shows it: +inf at an empty cell
__device__ __forceinline__ float ground_surface(const uint32_t word) {
  return word == kGroundEmpty ? __builtin_inff() : group_unkey_f32(word);
}

// what a morphology pass combines: a cell word read, and the result written back
template <bool kMax>
__device__ __forceinline__ uint32_t ground_morph_in(const uint32_t word) {
  return kMax && word == kGroundEmpty ? 0u : word;
}
template <bool kMax>
__device__ __forceinline__ uint32_t ground_morph_out(const uint32_t v) {
  return kMax && v == 0u ? kGroundEmpty : v;
}
template <bool kMax>
__device__ __forceinline__ uint32_t ground_morph_op(const uint32_t a, const uint32_t b) {
  return kMax ? (a > b ? a : b) : (a < b ? a : b);
}

// does a live point at height z over the cell word `word` (never empty: its own cell holds it) survive the window?
__device__ __forceinline__ bool ground_survives(const float z, const uint32_t word, const float height) {
  return z - group_unkey_f32(word) < height;
}
__device__ __forceinline__ float ground_hag(const float z, const uint32_t word) { return z - group_unkey_f32(word); }

}  // namespace pcgx
