// boundary_terms.h -- the decisions of boundary detection, shared by the device kernel (boundary.hip) and the host test
// (tests/cpp/boundary_terms_host.cpp): one expression, compiled by both.
// NOT in the reference: no parity, checked against the NumPy oracle's restatement (tests/boundary_oracle.py).
//
// Contract (include/pcgx.h, "boundary points"): float64 from widened float32, every product and sum rounded once in
// the written order, nothing fused (build with -ffp-contract=off, the rule of ref_dist_sq), no square root, no
// division and no table in memory: the tangents are literals chosen by selects.
#pragma once
#include "pcgx_math.h"

namespace pcgx {

constexpr int kBoundarySectors = 64;  // of 5.625 degrees each; the mask is one 64-bit word

// T[k], k = 1..15: the float64 nearest tan(k pi / 32); T[8] is 1 exactly.
#define PCGX_BOUNDARY_T1 0x1.936bb8c5b2da2p-4
#define PCGX_BOUNDARY_T2 0x1.975f5e0553158p-3
#define PCGX_BOUNDARY_T3 0x1.36a08355c63dcp-2
#define PCGX_BOUNDARY_T4 0x1.a827999fcef32p-2
#define PCGX_BOUNDARY_T5 0x1.11ab7190834ecp-1
#define PCGX_BOUNDARY_T6 0x1.561b82ab7f990p-1
#define PCGX_BOUNDARY_T7 0x1.a43002ae42850p-1
#define PCGX_BOUNDARY_T8 0x1.0000000000000p+0
#define PCGX_BOUNDARY_T9 0x1.37efd8d87607ep+0
#define PCGX_BOUNDARY_T10 0x1.7f218e25a7461p+0
#define PCGX_BOUNDARY_T11 0x1.def13b73c1406p+0
#define PCGX_BOUNDARY_T12 0x1.3504f333f9de6p+1
#define PCGX_BOUNDARY_T13 0x1.a5f59e90600ddp+1
#define PCGX_BOUNDARY_T14 0x1.41bfee2424771p+2
#define PCGX_BOUNDARY_T15 0x1.44e6c595afdccp+3

// T[k] for the host test's table (k = 1..15; anything else: 0)
PCGX_HD double boundary_tan(const int k) {
  switch (k) {
    case 1: return PCGX_BOUNDARY_T1;
    case 2: return PCGX_BOUNDARY_T2;
    case 3: return PCGX_BOUNDARY_T3;
    case 4: return PCGX_BOUNDARY_T4;
    case 5: return PCGX_BOUNDARY_T5;
    case 6: return PCGX_BOUNDARY_T6;
    case 7: return PCGX_BOUNDARY_T7;
    case 8: return PCGX_BOUNDARY_T8;
    case 9: return PCGX_BOUNDARY_T9;
    case 10: return PCGX_BOUNDARY_T10;
    case 11: return PCGX_BOUNDARY_T11;
    case 12: return PCGX_BOUNDARY_T12;
    case 13: return PCGX_BOUNDARY_T13;
    case 14: return PCGX_BOUNDARY_T14;
    case 15: return PCGX_BOUNDARY_T15;
    default: return 0.0;
  }
}

// Can a frame be built from this normal?  Three finite components, not all zero (either sign).
PCGX_HD bool boundary_normal_usable(const float nx, const float ny, const float nz) {
  const float big = 3.4028234663852886e38f;  // (NaN and +-inf fail the comparison)
  const bool finite = fabsf(nx) <= big && fabsf(ny) <= big && fabsf(nz) <= big;
  return finite && !(nx == 0.0f && ny == 0.0f && nz == 0.0f);
}

// Is point i evaluated?  It met itself in N(i), its normal is usable, and N(i) has max(min_neighbors, 1) members.
PCGX_HD bool boundary_evaluated(const bool met, const bool usable, const int32_t count, const int32_t min_neighbors) {
  return met && usable && count >= (min_neighbors > 1 ? min_neighbors : 1);
}

// The tangent frame of a normal: u = n x e and v = n x u, e the unit vector of the axis where |n| is smallest (a tie:
// the lowest axis).  float64 from the widened float32 components, not normalised: |u| = |n| sin(n, e), |v| = |n| |u|,
// so a normal of length L stretches v by L beside u and skews the sectors accordingly.
struct BoundaryFrame {
  double ux, uy, uz, vx, vy, vz;
};

PCGX_HD BoundaryFrame boundary_frame(const float fnx, const float fny, const float fnz) {
  const double nx = (double)fnx, ny = (double)fny, nz = (double)fnz;
  const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
  const int axis = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
  const double ex = axis == 0 ? 1.0 : 0.0, ey = axis == 1 ? 1.0 : 0.0, ez = axis == 2 ? 1.0 : 0.0;
  BoundaryFrame f;
  f.ux = ny * ez - nz * ey;
  f.uy = nz * ex - nx * ez;
  f.uz = nx * ey - ny * ex;
  f.vx = ny * f.uz - nz * f.uy;
  f.vy = nz * f.ux - nx * f.uz;
  f.vz = nx * f.uy - ny * f.ux;
  return f;
}

// a and b of neighbour p seen from q: d = p - q, a = (d.x u.x + d.y u.y) + d.z u.z, b likewise with v.
PCGX_HD void boundary_direction(const BoundaryFrame &f, const float px, const float py, const float pz, const float qx,
                                const float qy, const float qz, double &a, double &b) {
  const double dx = (double)px - (double)qx, dy = (double)py - (double)qy, dz = (double)pz - (double)qz;
  a = (dx * f.ux + dy * f.uy) + dz * f.uz;
  b = (dx * f.vx + dy * f.vy) + dz * f.vz;
}

// The sector 0..63 of the direction (a, b), both finite; -1 for a == b == 0 (the point itself, a coincident point, a
// point on the normal's line).  A sector owns its lower border.  A quarter turn brings the direction to x > 0, y >= 0;
// s = #{k in 1..15 : y >= x T[k]} by four comparisons, x T[k] being monotone in k.
PCGX_HD int boundary_sector(const double a, const double b) {
  if (a == 0.0 && b == 0.0) return -1;
  int q;
  double x, y;
  if (a > 0.0 && b >= 0.0) {
    q = 0, x = a, y = b;
  } else if (a <= 0.0 && b > 0.0) {
    q = 1, x = b, y = -a;
  } else if (a < 0.0 && b <= 0.0) {
    q = 2, x = -a, y = -b;
  } else {
    q = 3, x = -b, y = a;
  }
  int s = y >= x * PCGX_BOUNDARY_T8 ? 8 : 0;
  s += y >= x * (s ? PCGX_BOUNDARY_T12 : PCGX_BOUNDARY_T4) ? 4 : 0;
  const double t2 = s & 8 ? (s & 4 ? PCGX_BOUNDARY_T14 : PCGX_BOUNDARY_T10) : (s & 4 ? PCGX_BOUNDARY_T6 : PCGX_BOUNDARY_T2);
  s += y >= x * t2 ? 2 : 0;
  const double lo = s & 4 ? (s & 2 ? PCGX_BOUNDARY_T7 : PCGX_BOUNDARY_T5) : (s & 2 ? PCGX_BOUNDARY_T3 : PCGX_BOUNDARY_T1);
  const double hi = s & 4 ? (s & 2 ? PCGX_BOUNDARY_T15 : PCGX_BOUNDARY_T13) : (s & 2 ? PCGX_BOUNDARY_T11 : PCGX_BOUNDARY_T9);
  s += y >= x * (s & 8 ? hi : lo) ? 1 : 0;
  return 16 * q + s;
}

PCGX_HD uint64_t boundary_rotr(const uint64_t x, const int k) {  // k in 0..63
  return (x >> k) | (x << ((64 - k) & 63));
}

// The longest cyclic run of zero bits of mask: 0 for all ones, 64 for 0.  By doubling: r[j] has bit p set where 2^j
// zero bits begin at p (upwards, cyclically); the run is then grown greedily from the longest power down.  Six and six
// steps for every mask, no table.
PCGX_HD int boundary_gap(const uint64_t mask) {
  const uint64_t z = ~mask;
  if (z == ~(uint64_t)0) return 64;
  const uint64_t r0 = z;
  const uint64_t r1 = r0 & boundary_rotr(r0, 1);
  const uint64_t r2 = r1 & boundary_rotr(r1, 2);
  const uint64_t r3 = r2 & boundary_rotr(r2, 4);
  const uint64_t r4 = r3 & boundary_rotr(r3, 8);
  const uint64_t r5 = r4 & boundary_rotr(r4, 16);
  uint64_t cur = ~(uint64_t)0;  // bit p: `len` zero bits begin at p
  int len = 0;
  uint64_t t;
  t = cur & r5;  // (len is 0: no rotation)
  if (t) cur = t, len += 32;
  t = cur & boundary_rotr(r4, len);
  if (t) cur = t, len += 16;
  t = cur & boundary_rotr(r3, len);
  if (t) cur = t, len += 8;
  t = cur & boundary_rotr(r2, len);
  if (t) cur = t, len += 4;
  t = cur & boundary_rotr(r1, len);
  if (t) cur = t, len += 2;
  t = cur & boundary_rotr(r0, len);
  if (t) cur = t, len += 1;
  return len;
}

}  // namespace pcgx
