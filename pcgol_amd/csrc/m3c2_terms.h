// m3c2_terms.h -- the decisions of the cylinder statistics and of M3C2's finish, shared by the device kernels
// (m3c2.hip) and the host test (tests/cpp/m3c2_terms_host.cpp): one expression, compiled by both.
// NOT in the reference: no parity, checked against the NumPy oracle's restatement (tests/m3c2_oracle.py).
//
// Contract (include/pcgx.h, "cylinder statistics"): a cylinder is a ray's tube (ray_terms.h: o the core, d the axis,
// the same w, a, dd, cc) cut at both ends by a.a <= (L L) dd instead of by a parameter range.  float64 from widened
// float32, every product and sum rounded once in the written order, nothing fused, no square root and no division in
// what a result is made of.
//
// ---- the range.  ray_clip, ray_slabs, ray_border, ray_centre and ray_bound want a range [a_lo, a_hi] of a that holds
// every member; the cylinder hands them a_hi = sqrt((L L) dd) (1 + 2^-50), a_lo = -a_hi.  Why that is a superset of
// a.a <= (L L) dd: the rounded a.a is at least a^2 (1 - 2^-53) (an a.a that underflows has |a| < 2^-511, below every
// a_hi: (L L) dd >= 2^-596), so |a| <= sqrt((L L) dd) (1 + 2^-52), and the root's and the product's two roundings take
// less than 2^-52 off 1 + 2^-50.  cyl_member is ray_member over that range AND the contract's a.a <= (L L) dd: the
// range decides nothing, and the cover proof of ray_terms.h ("the clip", "the cover") applies unchanged, its [s_min dd,
// s_max dd] being any interval that holds the members' a.
#pragma once
#include "ray_terms.h"

namespace pcgx {

struct Cyl {
  Ray r;        // usable: core and axis finite, dd != 0
  double lldd;  // (L L) dd
};

PCGX_HD Cyl cyl_make(const float ox, const float oy, const float oz, const float dx, const float dy, const float dz,
                     const float rho, const float half_length) {
  Cyl c;
  c.r = ray_make(ox, oy, oz, dx, dy, dz, -__builtin_inff(), __builtin_inff(), rho);
  const double ll = (double)half_length * (double)half_length;
  c.lldd = ll * c.r.dd;
  c.r.a_hi = sqrt(c.lldd) * (1.0 + 0x1p-50);
  c.r.a_lo = -c.r.a_hi;
  return c;
}

// Is the point a member of the cylinder?  a is what the sums are made of.
PCGX_HD bool cyl_member(const Cyl &c, const float px, const float py, const float pz, double &a, double &cc) {
  return ray_member(c.r, px, py, pz, a, cc) && a * a <= c.lldd;
}

// How many slabs a cylinder has at most, from L, the slab length `target` and nothing else: ray_slabs of a range no
// longer than 2 a_hi.  (0x1p-40 stands above a_hi's 2^-50, the clip's, the quotient's and this line's own roundings.)
inline double cyl_slab_bound(const float half_length, const float target) {
  return (2.0 * (double)half_length * (1.0 + 0x1p-40)) / (double)target + 1.0;
}

// M3C2's finish for one core (include/pcgx.h, "M3C2"): float64 in the written order, IEEE division and square root.
struct M3C2Value {
  double distance, lod;
  uint8_t significant;
};

PCGX_HD double m3c2_variance(const double n, const double s1, const double s2, const double dd) {
  const double v = (s2 - (s1 * s1) / n) / (n - 1.0);
  return (v > 0.0 ? v : 0.0) / dd;  // (a NaN too is 0)
}

PCGX_HD M3C2Value m3c2_finish(const float dx, const float dy, const float dz, const int32_t n1, const double s1_1,
                              const double s2_1, const int32_t n2, const double s1_2, const double s2_2,
                              const double registration_error, const int32_t min_count) {
  const double x = (double)dx, y = (double)dy, z = (double)dz;
  const double dd = (x * x + y * y) + z * z;
  M3C2Value v;
  v.distance = v.lod = __builtin_nan("");
  v.significant = 0;
  if (!(ray_finite(dx) && ray_finite(dy) && ray_finite(dz)) || dd == 0.0 || n1 < min_count || n2 < min_count) return v;
  const double m1 = (double)n1, m2 = (double)n2;
  const double mean1 = s1_1 / m1, mean2 = s1_2 / m2;
  const double var1 = m3c2_variance(m1, s1_1, s2_1, dd), var2 = m3c2_variance(m2, s1_2, s2_2, dd);
  v.distance = (mean2 - mean1) / sqrt(dd);
  v.lod = 1.96 * (sqrt(var1 / m1 + var2 / m2) + registration_error);
  v.significant = fabs(v.distance) > v.lod ? 1 : 0;
  return v;
}

}  // namespace pcgx
