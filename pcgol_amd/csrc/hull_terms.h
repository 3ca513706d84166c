// hull_terms.h -- the decisions of per-group footprints, shared by the device kernels (group_hull.hip) and the host test
// (tests/cpp/hull_terms_host.cpp over the shim tests/cpp/host_shim): one expression, compiled by both.
// NOT in the reference: no parity, checked against the exact oracle (tests/hull_oracle.py).
//
// Contract (include/pcgx.h, "group footprints"): the place of a member and its lexicographic key, the exact
// orientation test for float32 points, the shoelace term of the area and one edge's rectangle from running extents.
#pragma once
#include "group_terms.h"

namespace pcgx {

// ------------------------------------------------------------------ places and their keys
// -0 -> +0, every other value as it is: `==` calls the two zeros equal, so a place needs one key for both.
__device__ __forceinline__ float hull_canon(const float v) {
  uint32_t b;
  __builtin_memcpy(&b, &v, 4);
  if (b == 0x80000000u) b = 0u;
  float r;
  __builtin_memcpy(&r, &b, 4);
  return r;
}
// Are two members at the same place?  (finite coordinates: a live member's)
__device__ __forceinline__ bool hull_same_place(const float ax, const float ay, const float bx, const float by) {
  return ax == bx && ay == by;
}
// The lexicographic key of the place (x, y): group_key_f32(x) high, group_key_f32(y) low, both zeros canonicalised to
// +0 first -- group_key_f32 alone sorts -0 below +0, which would split one place in two.  a < b lexicographically
// <=> key(a) < key(b); the same place <=> the same key.
__device__ __forceinline__ uint64_t hull_key(const float x, const float y) {
  return ((uint64_t)group_key_f32(hull_canon(x)) << 32) | (uint64_t)group_key_f32(hull_canon(y));
}
__device__ __forceinline__ float hull_key_x(const uint64_t k) { return group_unkey_f32((uint32_t)(k >> 32)); }
__device__ __forceinline__ float hull_key_y(const uint64_t k) { return group_unkey_f32((uint32_t)k); }

// ------------------------------------------------------------------ the orientation test
#if defined(PCGX_HULL_HOST_COUNT)
static long long g_hull_orient_fallbacks = 0;  // host build only: how often the exact branch answered
#endif

// s + e = a + b exactly (Knuth); additions only, nothing a compiler could contract
__device__ __forceinline__ void hull_two_sum(const double a, const double b, double &s, double &e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// The exact sign of (ax - cx)(by - cy) - (ay - cy)(bx - cx) = ax by - ax cy - cx by - ay bx + ay cx + cy bx: six
// products of two float32 values, each exact in float64 (48 significant bits, no under- or overflow: 2^-298 <= |p| <
// 2^256), added into a non-overlapping expansion by Shewchuk's Grow-Expansion with fixed, unrolled indices; the sign of
// the sum is the sign of the expansion's most significant non-zero component.  A product fused into the first addition
// of its two-sum is rounded once from the same exact value: the outcome does not depend on FMA contraction.
__device__ __forceinline__ int hull_orient_exact(const float ax, const float ay, const float bx, const float by,
                                                 const float cx, const float cy) {
  const double p0 = (double)ax * (double)by, p1 = -((double)ax * (double)cy), p2 = -((double)cx * (double)by);
  const double p3 = -((double)ay * (double)bx), p4 = (double)ay * (double)cx, p5 = (double)cy * (double)bx;
  double h0, h1, h2, h3, h4, h5, q;
  h0 = p0;
  q = p1; hull_two_sum(q, h0, q, h0); h1 = q;
  q = p2; hull_two_sum(q, h0, q, h0); hull_two_sum(q, h1, q, h1); h2 = q;
  q = p3; hull_two_sum(q, h0, q, h0); hull_two_sum(q, h1, q, h1); hull_two_sum(q, h2, q, h2); h3 = q;
  q = p4; hull_two_sum(q, h0, q, h0); hull_two_sum(q, h1, q, h1); hull_two_sum(q, h2, q, h2); hull_two_sum(q, h3, q, h3);
  h4 = q;
  q = p5; hull_two_sum(q, h0, q, h0); hull_two_sum(q, h1, q, h1); hull_two_sum(q, h2, q, h2); hull_two_sum(q, h3, q, h3);
  hull_two_sum(q, h4, q, h4);
  h5 = q;
  const double top = h5 != 0.0 ? h5 : (h4 != 0.0 ? h4 : (h3 != 0.0 ? h3 : (h2 != 0.0 ? h2 : (h1 != 0.0 ? h1 : h0))));
  return top > 0.0 ? 1 : (top < 0.0 ? -1 : 0);
}

// -1 / 0 / +1: c right of, on, left of the line from a to b -- the exact sign of the determinant above for finite
// float32 inputs.  First the float64 evaluation with Shewchuk's static bound (3 + 16 eps) eps (|l| + |r|), eps = 2^-53
// (the differences are rounded at most once each, the bound is his ccwerrboundA); where the bound does not certify the
// sign, the exact sum.
__device__ __forceinline__ int hull_orient(const float ax, const float ay, const float bx, const float by, const float cx,
                                           const float cy) {
  const double l = ((double)ax - (double)cx) * ((double)by - (double)cy);
  const double r = ((double)ay - (double)cy) * ((double)bx - (double)cx);
  const double det = l - r;
  const double eps = 1.1102230246251565e-16;  // 2^-53
  const double bound = ((3.0 + 16.0 * eps) * eps) * (fabs(l) + fabs(r));
  if (det > bound) return 1;
  if (-det > bound) return -1;
#if defined(PCGX_HULL_HOST_COUNT)
  g_hull_orient_fallbacks++;
#endif
  return hull_orient_exact(ax, ay, bx, by, cx, cy);
}

// ------------------------------------------------------------------ area
// One term of the fan about v0: cross(a - v0, b - v0), the differences in float64
__device__ __forceinline__ double hull_shoelace(const float v0x, const float v0y, const float ax, const float ay,
                                                const float bx, const float by) {
  const double ux = (double)ax - (double)v0x, uy = (double)ay - (double)v0y;
  const double wx = (double)bx - (double)v0x, wy = (double)by - (double)v0y;
  return ux * wy - uy * wx;
}

// ------------------------------------------------------------------ one edge's rectangle
// The extents of the vertices along u and n = (-u_y, u_x), measured from the edge's first vertex o (itself at 0, 0).
struct HullExtents {
  double ox, oy, ux, uy;       // the edge's first vertex and its unit direction
  double lo_u, hi_u, lo_n, hi_n;
  // the edge from o to b (two places: a non-zero length); u = (b - o) / |b - o| in float64
  __device__ __forceinline__ void start(const float ox_, const float oy_, const float bx, const float by) {
    ox = (double)ox_;
    oy = (double)oy_;
    const double dx = (double)bx - ox, dy = (double)by - oy;
    const double len = sqrt(dx * dx + dy * dy);
    ux = dx / len;
    uy = dy / len;
    lo_u = hi_u = lo_n = hi_n = 0.0;
  }
  __device__ __forceinline__ void add(const float px, const float py) {
    const double dx = (double)px - ox, dy = (double)py - oy;
    const double s = dx * ux + dy * uy, t = dy * ux - dx * uy;
    lo_u = s < lo_u ? s : lo_u;
    hi_u = s > hi_u ? s : hi_u;
    lo_n = t < lo_n ? t : lo_n;
    hi_n = t > hi_n ? t : hi_n;
  }
  // the product of the two widths: what the edges are compared by
  __device__ __forceinline__ double area() const { return (hi_u - lo_u) * (hi_n - lo_n); }
  // centre x, y; u; the half-extents along u and n
  __device__ __forceinline__ void rect(double (&out)[6]) const {
    const double mu = (hi_u + lo_u) * 0.5, mn = (hi_n + lo_n) * 0.5;
    out[0] = ox + (mu * ux - mn * uy);
    out[1] = oy + (mu * uy + mn * ux);
    out[2] = ux;
    out[3] = uy;
    out[4] = (hi_u - lo_u) * 0.5;
    out[5] = (hi_n - lo_n) * 0.5;
  }
};

}  // namespace pcgx
