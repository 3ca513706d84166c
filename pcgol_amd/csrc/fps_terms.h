// fps_terms.h -- the decisions of farthest-point sampling, shared by the device kernels (fps.hip) and the host test
// (tests/cpp/fps_terms_host.cpp): one expression, compiled by both, never contracted (-ffp-contract=off, the rule of
// ref_dist_sq).  NOT in the reference: no parity, checked against the NumPy oracle's restatement (tests/fps_oracle.py).
//
// Contract (include/pcgx.h, "farthest-point sampling"): pick j+1 is the eligible, not yet picked point with the largest
// d_j(p) = min over the picks so far of DistSq(p, pick), ties to the smallest id.  d is kept as a running minimum with
// the STRICT update nd < d, so a point's owner is the earliest of its nearest picks.
//
// The box lemma (what lets a pick skip a tile of points).  Let lo <= p <= hi componentwise, all finite, and s finite.
//   c = clamp(s, lo, hi) componentwise, fps_box_lower(s, lo, hi) = ref_dist_sq(c, s).
// Claim: fps_box_lower(s, lo, hi) <= ref_dist_sq(p, s) IN FLOAT32, EXACTLY, at any coordinates.
//   1. Per axis k the real numbers satisfy |p_k - s_k| >= |c_k - s_k|, and the two differences have the same sign or
//      the second is 0: s_k < lo_k gives c_k = lo_k <= p_k, so p_k - s_k >= c_k - s_k > 0; s_k > hi_k mirrors it; s_k
//      inside gives c_k = s_k and c_k - s_k = 0.
//   2. Round-to-nearest is monotone (x <= y implies fl(x) <= fl(y)) and odd, so |fl(p_k - s_k)| >= |fl(c_k - s_k)|.
//   3. Squaring a float32 is the monotone map |x| -> fl(x * x): dp_k^2 >= dc_k^2 as float32, +inf included.
//   4. Float32 addition is monotone in either operand, and the two sums are formed in the same order
//      (dx dx + dy dy) + dz dz: the sum over p is >= the sum over c.  No step produces a NaN: every term is >= +0 or
//      +inf, and inf - inf never arises.
// So a tile whose box has fps_box_lower >= the largest d among its members holds no member with nd < d: the strict
// update changes nothing there, and d, owners and keys stay what the plain loop over every point gives.
#pragma once
#include "pcgx_math.h"

namespace pcgx {

// bits of a float32 and back
PCGX_HD uint32_t fps_bits(const float f) { return __builtin_bit_cast(uint32_t, f); }
PCGX_HD float fps_from_bits(const uint32_t u) { return __builtin_bit_cast(float, u); }

// Is the point in E as far as its coordinates go?  (A deleted point is in no tree: the gather never sees it.)
PCGX_HD bool fps_finite(const float v) { return v - v == 0.0f; }
PCGX_HD bool fps_eligible(const float x, const float y, const float z) { return fps_finite(x) && fps_finite(y) && fps_finite(z); }

// The distance is ref_dist_sq (pcgx_math.h), the reference's float32 DistSq: p - q, then (dx dx + dy dy) + dz dz.  It is
// symmetric bit for bit: fl(a - b) = -fl(b - a).

// The pick key: one unsigned maximum gives "largest d, then smallest id".  d is >= +0 and no NaN on E, where the bits
// of a float32 order as the values do; ids are below 2^31, so the low word is never 0 and a key of 0 can stand for
// "picked, or not eligible".
constexpr uint32_t kFpsMaxId = 0x7ffffffeu;
PCGX_HD uint64_t fps_key(const float d, const uint32_t id) { return ((uint64_t)fps_bits(d) << 32) | (uint64_t)(0xffffffffu - id); }
PCGX_HD uint32_t fps_key_id(const uint64_t key) { return 0xffffffffu - (uint32_t)key; }
PCGX_HD float fps_key_d(const uint64_t key) { return fps_from_bits((uint32_t)(key >> 32)); }

// The strict update of the running minimum: an owner changes only when a later pick is strictly nearer.
PCGX_HD bool fps_updates(const float nd, const float d) { return nd < d; }

// The least DistSq any point of the box [lo, hi] can have to s (the lemma above).  The clamp selects one of its three
// operands: nothing is rounded.
PCGX_HD float fps_clamp(const float s, const float lo, const float hi) { return s < lo ? lo : (s > hi ? hi : s); }
PCGX_HD float fps_box_lower(const float sx, const float sy, const float sz, const float lox, const float loy,
                            const float loz, const float hix, const float hiy, const float hiz) {
  return ref_dist_sq(fps_clamp(sx, lox, hix), fps_clamp(sy, loy, hiy), fps_clamp(sz, loz, hiz), sx, sy, sz);
}

// May a pick at s leave the tile alone?  max_d: the largest d among the tile's candidates (the d word of its key; 0
// where it has none, and then nothing in it can decrease).  An empty tile's box of (+inf, -inf) clamps s to +inf: the
// bound is +inf and the tile is skipped.  A NaN bound, should one ever arise, compares false and the tile is touched:
// touching is always right, skipping is what needs the lemma.
PCGX_HD bool fps_skips(const float lower, const float max_d) { return lower >= max_d; }

// what the outputs hold where there is no pick
constexpr int32_t kFpsNoId = -1;
constexpr float kFpsNoDist = -1.0f;

}  // namespace pcgx
