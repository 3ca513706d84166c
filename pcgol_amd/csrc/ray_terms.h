// ray_terms.h -- the decisions of the ray queries, shared by the device kernel (rays.hip) and the host test
// (tests/cpp/ray_terms_host.cpp): one expression, compiled by both.
// NOT in the reference: no parity, checked against the NumPy oracle's restatement (tests/rays_oracle.py).
//
// Contract (include/pcgx.h, "ray queries"): float64 from widened float32, every product and sum rounded once in the
// written order, nothing fused (build with -ffp-contract=off, the rule of ref_dist_sq).  What a result is made of --
// the member test, `along`, `off_sq`, the comparison -- has no square root and no division.  The clip and the cover
// below only choose which records are LOOKED AT; they divide and take roots (IEEE, correctly rounded on both sides),
// and what they owe is a superset, proven here.
//
// ---- the clip.  Every member p lies in the box [lo, hi] of the tree's finite points.  Let M = max(|o|, |lo|, |hi|)
// over all components, u = 2^-20, pad = rho (1 + u) + u M.  ray_clip intersects the ray with the box inflated by pad,
// axis by axis in s (a slab test), and returns the range in a = s dd, cut to [s_min dd, s_max dd] by the member test's
// own two products.  Why no member is lost: the computed a and cc of a member differ from the real w.d and |w x d|^2
// by the rounding of at most five float64 operations on terms no larger than |w| |d|, |w| <= 2 sqrt(3) M.  So the real
// foot f = o + (a / dd) d lies within rho (1 + 2^-50) + 2^-47 M of p, which is inside the box: f is inside the box
// inflated by that much, and its s inside that box's real slab range.  The computed range comes from (face - o) / d
// with face = lo - pad or hi + pad: three roundings, each worth moving the face by at most 2^-50 (M + pad).  pad
// exceeds what is needed by u M - 2^-47 M - 2^-49 (M + pad): 27 bits to spare.
//
// ---- the cover.  [A0, A1] is cut into K slabs at b_k = min(A0 + (A1 - A0) (k / K), A1), b_0 = A0, b_K = A1
// (ray_border: monotone in k since k / K, the product and the sum are).  Slab k owns a in [b_k, b_k+1), the last one
// [b_K-1, b_K]: every a in [A0, A1] has exactly one owner (ray_in_slab).  Its ball: m = (b_k + b_k+1) / 2, centre
// c = float32(clamp(o + (m / dd) d, lo, hi)) (ray_centre), and with half = (A1 - A0) / (2 K sqrt(dd)), every slab's
// metric half length up to two ulps of a border (ray_bound: one bound for all slabs of a ray)
//     R = sqrt((rho (1 + u) + u M)^2 + (half (1 + u) + u M)^2) + u M,   bound = float32(R^2 (1 + 2^-18) (1 + u)),
// at least kRayBoundFloor and at most FLT_MAX.  Claim: a member p owned by slab k has ref_dist_sq(p, c) < bound.
//   1. In reals, with c* = o + (m / dd) d: |p - c*|^2 = r^2 + l^2, r the distance from p to the line, l the distance
//      along it.  r <= rho (1 + 2^-50) + 2^-47 M as above.  l = |w.d - m| / |d| <= (|a - m| + 2^-50 |w| |d|) / |d|,
//      and |a - m| <= (A1 - A0) / (2 K) + 3 ulp(m), ulp(m) / |d| <= 2^-52 |c* - o| <= 2^-49 (M + rho).  So r <= rho (1 + u) + u M
//      and l <= half (1 + u) + u M with room for half's own three roundings.
//   2. The computed float64 centre is within 2^-49 (M + rho) of c* (c* lies in the inflated box; rho (1 + u) in R has
//      u rho to spare for it).  Clamping to the box moves it no farther from any point
//      of the box, p among them.  Rounding to float32 moves it by at most 2^-24 M per axis, sqrt(3) 2^-24 M < u M / 9
//      in all (and keeps it in the box, lo and hi being float32).  So |p - c| <= R - u M / 2.
//   3. ref_dist_sq is five float32 operations, each at most 1 + 2^-24 above the real one: the computed value is at most
//      |p - c|^2 (1 + 2^-21), plus 2^-148 where a term is denormal.  bound >= R^2 (1 + 2^-18) after its own rounding,
//      and the floor stands above what denormals add: the comparison is strict.
//   4. Overflow.  c lies in the box, so a difference is at most the box's extent E; pcgx_kdtree_raycast refuses a tree
//      with E >= 2^62 (kRayMaxExtent), where 3 E^2 (1 + 2^-21) would not stay below FLT_MAX.  A bound beyond FLT_MAX
//      becomes FLT_MAX: the ball is then the whole tree.  Every float64 term is at most 2^128 2^128 2^20.
// The margin grows with M because the float32 centre does: at M = 4096 it is 2^-8 wide, a quarter of rho = 2^-6.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pcgx_math.h"

namespace pcgx {

constexpr int kRaySlabCap = 4096;  // slabs per ray at most: longer slabs beyond, never a shorter ray
#define PCGX_RAY_U 0x1p-20
#define PCGX_RAY_FLT_MAX 0x1.fffffep+127
constexpr float kRayBoundFloor = 0x1p-120f;
constexpr float kRayMaxExtent = 0x1p62f;

struct Ray {
  double ox, oy, oz, dx, dy, dz;
  double dd;        // (d.x d.x + d.y d.y) + d.z d.z
  double rrdd;      // (rho rho) dd
  double a_lo, a_hi;  // s_min dd, s_max dd
  bool usable;
};

PCGX_HD bool ray_finite(const float v) { return fabsf(v) <= 3.4028234663852886e38f; }  // (NaN fails the comparison)

// s_min, s_max: NULL in the ABI is 0 and +inf here
PCGX_HD Ray ray_make(const float ox, const float oy, const float oz, const float dx, const float dy, const float dz,
                     const float s_min, const float s_max, const float rho) {
  Ray r;
  r.ox = (double)ox, r.oy = (double)oy, r.oz = (double)oz;
  r.dx = (double)dx, r.dy = (double)dy, r.dz = (double)dz;
  r.dd = (r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz;
  const double rr = (double)rho * (double)rho;
  r.rrdd = rr * r.dd;
  r.a_lo = (double)s_min * r.dd;
  r.a_hi = (double)s_max * r.dd;
  const bool finite = ray_finite(ox) && ray_finite(oy) && ray_finite(oz) && ray_finite(dx) && ray_finite(dy) && ray_finite(dz);
  r.usable = finite && r.dd != 0.0 && s_min == s_min && s_max == s_max && !(s_min > s_max);
  return r;
}

// Is the point a member of the ray?  a and cc are what the results carry.
PCGX_HD bool ray_member(const Ray &r, const float px, const float py, const float pz, double &a, double &cc) {
  const double wx = (double)px - r.ox, wy = (double)py - r.oy, wz = (double)pz - r.oz;
  a = (wx * r.dx + wy * r.dy) + wz * r.dz;
  const double cx = wy * r.dz - wz * r.dy, cy = wz * r.dx - wx * r.dz, cz = wx * r.dy - wy * r.dx;
  cc = (cx * cx + cy * cy) + cz * cz;
  const bool finite = ray_finite(px) && ray_finite(py) && ray_finite(pz);
  return r.usable && finite && cc <= r.rrdd && r.a_lo <= a && a <= r.a_hi;
}

// Does the hit (a, id) beat (b, jd)?  id < 0: no hit.
PCGX_HD bool ray_beats(const double a, const int32_t id, const double b, const int32_t jd) {
  if (id < 0) return false;
  if (jd < 0) return true;
  return a < b || (a == b && id < jd);
}

// The box of the tree's finite points, and M's share of it
struct RayBox {
  float lo[3], hi[3];
  bool any;  // a finite point exists
};

PCGX_HD double ray_magnitude(const Ray &r, const RayBox &b) {
  double m = fmax(fmax(fabs(r.ox), fabs(r.oy)), fabs(r.oz));
#pragma unroll
  for (int k = 0; k < 3; k++) m = fmax(m, fmax(fabs((double)b.lo[k]), fabs((double)b.hi[k])));
  return m;
}

// [a0, a1]: where in a = s dd the members can lie.  false: nowhere.
PCGX_HD bool ray_clip(const Ray &r, const RayBox &b, const float rho, double &a0, double &a1) {
  a0 = 0.0, a1 = 0.0;
  if (!r.usable || !b.any) return false;
  const double pad = (double)rho * (1.0 + PCGX_RAY_U) + PCGX_RAY_U * ray_magnitude(r, b);
  const double o[3] = {r.ox, r.oy, r.oz}, d[3] = {r.dx, r.dy, r.dz};
  double s0 = -HUGE_VAL, s1 = HUGE_VAL;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double f0 = (double)b.lo[k] - pad, f1 = (double)b.hi[k] + pad;
    if (d[k] == 0.0) {
      if (o[k] < f0 || o[k] > f1) return false;
      continue;
    }
    const double t0 = (f0 - o[k]) / d[k], t1 = (f1 - o[k]) / d[k];
    s0 = fmax(s0, fmin(t0, t1));
    s1 = fmin(s1, fmax(t0, t1));
  }
  a0 = fmax(s0 * r.dd, r.a_lo);
  a1 = fmin(s1 * r.dd, r.a_hi);
  return a0 <= a1;
}

// How many slabs [a0, a1] is cut into: of metric length `target` (2 rho, or the grid's cell edge where that is longer),
// kRaySlabCap at most.
PCGX_HD int32_t ray_slabs(const Ray &r, const double a0, const double a1, const float target) {
  const double q = ((a1 - a0) / sqrt(r.dd)) / (double)target;
  return q >= (double)(kRaySlabCap - 1) ? kRaySlabCap : (int32_t)q + 1;  // (a NaN q: one slab)
}

// b_k, k = 0 .. K
PCGX_HD double ray_border(const double a0, const double a1, const int32_t k, const int32_t K) {
  if (k <= 0) return a0;
  if (k >= K) return a1;
  return fmin(a0 + (a1 - a0) * ((double)k / (double)K), a1);
}

// Does slab k own a?
PCGX_HD bool ray_in_slab(const double a, const double a0, const double a1, const int32_t k, const int32_t K) {
  const double b0 = ray_border(a0, a1, k, K), b1 = ray_border(a0, a1, k + 1, K);
  return b0 <= a && (a < b1 || (k == K - 1 && a <= b1));
}

// The ball query that reports every member slab k owns: its float32 centre ...
PCGX_HD void ray_centre(const Ray &r, const RayBox &b, const double a0, const double a1, const int32_t k, const int32_t K,
                        float &cx, float &cy, float &cz) {
  const double b0 = ray_border(a0, a1, k, K), b1 = ray_border(a0, a1, k + 1, K);
  const double s = (0.5 * (b0 + b1)) / r.dd;
  const double x = r.ox + s * r.dx, y = r.oy + s * r.dy, z = r.oz + s * r.dz;
  cx = (float)fmin(fmax(x, (double)b.lo[0]), (double)b.hi[0]);
  cy = (float)fmin(fmax(y, (double)b.lo[1]), (double)b.hi[1]);
  cz = (float)fmin(fmax(z, (double)b.lo[2]), (double)b.hi[2]);
}

// ... and the strict bound of ref_dist_sq, one for all K slabs of the ray (the visitor shares fat rows out under the
// calling lane's bound, so a wave's lanes must agree on it).
PCGX_HD float ray_bound(const Ray &r, const RayBox &b, const float rho, const double a0, const double a1, const int32_t K) {
  const double um = PCGX_RAY_U * ray_magnitude(r, b);
  const double half = ((0.5 * (a1 - a0)) / (double)K) / sqrt(r.dd);
  const double rp = (double)rho * (1.0 + PCGX_RAY_U) + um, hp = half * (1.0 + PCGX_RAY_U) + um;
  const double R = sqrt(rp * rp + hp * hp) + um;
  const double bd = (R * R) * (1.0 + 0x1p-18) * (1.0 + PCGX_RAY_U);
  return bd >= PCGX_RAY_FLT_MAX ? (float)PCGX_RAY_FLT_MAX : fmaxf((float)bd, kRayBoundFloor);
}

}  // namespace pcgx
