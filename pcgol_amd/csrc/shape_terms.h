// shape_terms.h -- the sphere or cylinder of two oriented points, the tests a hypothesis passes before it gets one, the
// partner rule's mix, the inlier test and the one refit, shared by the device kernels (shapes.hip) and the host test
// (tests/cpp/shape_terms_host.cpp): one expression, compiled by both.  NOT in the reference: no parity, checked against
// the NumPy oracle's restatement (tests/shape_oracle.py).
//
// Contract (include/pcgx.h, "shapes").  The hypothesis and the refit are float64 from the float32 points and normals,
// each operation rounded once; the inlier test is float32 with no square root; build with -ffp-contract=off.
//   mix        x = u1 ^ (id * 0x9E3779B1); x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
//              (uint32): the partner of a seed is the candidate with the smallest (x << 32) | id
//   status     1: no partner, or the partner is the seed; 2: den = A C - B B is not > 1e-12 (A C) (the normals are
//              parallel); 3: the axis test fails (cylinder); 4: the radius test fails or the record is not finite
//   lines      w = p0 - p1, A = n0.n0, B = n0.n1, C = n1.n1, D = n0.w, E = n1.w, s = (B E - C D) / den,
//              t = (A E - B D) / den, c0 = p0 + s n0, c1 = p1 + t n1, m = 0.5 (c0 + c1); dots are (x x + y y) + z z
//   sphere     centre m, r = 0.5 (|p0 - m| + |p1 - m|)
//   cylinder   a = n0 x n1 / |n0 x n1|, plane_axis_ok (|a . axis| >= cos |axis|: PARALLEL to the axis), plane_orient,
//              q = m - (m.a) a, r = 0.5 (rho(p0) + rho(p1)), rho(p) = sqrt(max(0, |v|^2 - (v.a)^2)), v = p - q
//   record     8 float32, each number rounded once: {cx, cy, cz, r, 0, 0, 0, 0} / {qx, qy, qz, r, ax, ay, az, 0}
//   inlier     lo = r - max_dist, hi = r + max_dist, hi2 = hi hi, lo2 = lo > 0 ? lo lo : -1, c2 = cos cos; v = p - centre;
//              sphere d2 = |v|^2, g = m.v; cylinder t = v.a, d2 = |v|^2 - t t, g = m.v - t (m.a);
//              d2 < hi2 && d2 > lo2 && (cos == 0 || g g >= c2 d2)
//   refit      Kasa's circle / sphere about the record's own centre (shape_refit below)
#pragma once
#include "plane_terms.h"

namespace pcgx {

constexpr int32_t kShapeSphere = 0, kShapeCylinder = 1;
constexpr int32_t kShapeNotRun = -1, kShapeOk = 0, kShapeNoPartner = 1, kShapeDegenerate = 2, kShapeAxis = 3,
                  kShapeRadius = 4;
constexpr int kShapeSums = 13;  // sum x [3], sum x x^T [6: xx xy xz yy yz zz], sum |x|^2 x [3], sum |x|^2

PCGX_HD uint32_t shape_mix(uint32_t u1, uint32_t id) {
  uint32_t x = u1 ^ (id * 0x9E3779B1u);
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}
PCGX_HD uint64_t shape_partner_key(uint32_t u1, uint32_t id) { return ((uint64_t)shape_mix(u1, id) << 32) | (uint64_t)id; }

PCGX_HD double shape_dot(double ax, double ay, double az, double bx, double by, double bz) {
  return (ax * bx + ay * by) + az * bz;
}
PCGX_HD double shape_pos(double v) { return v > 0.0 ? v : 0.0; }  // max(0, v); a NaN gives 0

PCGX_HD bool shape_radius_ok(double r, float r_min, float r_max) { return r >= (double)r_min && r <= (double)r_max; }

// the eight numbers rounded to float32: are they all finite?  (rec all zero and false otherwise)
PCGX_HD bool shape_store(const double *v8, float *rec8) {
  bool ok = true;
  for (int k = 0; k < 8; k++) {
    rec8[k] = (float)v8[k];
    ok = ok && plane_finite(rec8[k]);
  }
  if (!ok)
    for (int k = 0; k < 8; k++) rec8[k] = 0.0f;
  return ok;
}

// rho(p): the distance of p from the axis through q along the unit a
PCGX_HD double shape_rho(const double *p, const double *q, const double *a) {
  const double vx = p[0] - q[0], vy = p[1] - q[1], vz = p[2] - q[2];
  const double t = shape_dot(vx, vy, vz, a[0], a[1], a[2]);
  return sqrt(shape_pos(shape_dot(vx, vy, vz, vx, vy, vz) - t * t));
}

// q = c - (c.a) a: the point of the axis through c nearest the origin
PCGX_HD void shape_canonical(const double *c, const double *a, double *q) {
  const double t = shape_dot(c[0], c[1], c[2], a[0], a[1], a[2]);
  q[0] = c[0] - t * a[0];
  q[1] = c[1] - t * a[1];
  q[2] = c[2] - t * a[2];
}

// The hypothesis of the oriented points (p0, n0) and (p1, n1), partner false where the seed has none (or it is the
// seed): its status, and for kShapeOk its record (all zero otherwise).
PCGX_HD int32_t shape_hypothesis(int32_t kind, bool partner, const float *p0f, const float *n0f, const float *p1f,
                                 const float *n1f, const PlaneAxis &Ax, float r_min, float r_max, float *rec8) {
  for (int k = 0; k < 8; k++) rec8[k] = 0.0f;
  if (!partner) return kShapeNoPartner;
  double p0[3], p1[3], n0[3], n1[3], w[3];
  for (int k = 0; k < 3; k++) {
    p0[k] = (double)p0f[k];
    p1[k] = (double)p1f[k];
    n0[k] = (double)n0f[k];
    n1[k] = (double)n1f[k];
    w[k] = p0[k] - p1[k];
  }
  const double A = shape_dot(n0[0], n0[1], n0[2], n0[0], n0[1], n0[2]), B = shape_dot(n0[0], n0[1], n0[2], n1[0], n1[1], n1[2]),
               C = shape_dot(n1[0], n1[1], n1[2], n1[0], n1[1], n1[2]), D = shape_dot(n0[0], n0[1], n0[2], w[0], w[1], w[2]),
               E = shape_dot(n1[0], n1[1], n1[2], w[0], w[1], w[2]);
  const double den = A * C - B * B;
  if (!(den > 1e-12 * (A * C))) return kShapeDegenerate;
  const double s = (B * E - C * D) / den, t = (A * E - B * D) / den;
  double m[3];
  for (int k = 0; k < 3; k++) m[k] = 0.5 * ((p0[k] + s * n0[k]) + (p1[k] + t * n1[k]));
  double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double r;
  if (kind == kShapeSphere) {
    const double ux = p0[0] - m[0], uy = p0[1] - m[1], uz = p0[2] - m[2];
    const double vx = p1[0] - m[0], vy = p1[1] - m[1], vz = p1[2] - m[2];
    r = 0.5 * (sqrt(shape_dot(ux, uy, uz, ux, uy, uz)) + sqrt(shape_dot(vx, vy, vz, vx, vy, vz)));
    v[0] = m[0];
    v[1] = m[1];
    v[2] = m[2];
  } else {
    const double cx = n0[1] * n1[2] - n0[2] * n1[1], cy = n0[2] * n1[0] - n0[0] * n1[2], cz = n0[0] * n1[1] - n0[1] * n1[0];
    const double len = sqrt(shape_dot(cx, cy, cz, cx, cy, cz));
    double a[3] = {cx / len, cy / len, cz / len};
    if (!plane_axis_ok(a[0], a[1], a[2], Ax)) return kShapeAxis;
    plane_orient(a[0], a[1], a[2], Ax);
    double q[3];
    shape_canonical(m, a, q);
    r = 0.5 * (shape_rho(p0, q, a) + shape_rho(p1, q, a));
    v[0] = q[0];
    v[1] = q[1];
    v[2] = q[2];
    v[4] = a[0];
    v[5] = a[1];
    v[6] = a[2];
  }
  v[3] = r;
  if (!shape_radius_ok(r, r_min, r_max)) return kShapeRadius;
  if (!shape_store(v, rec8)) return kShapeRadius;
  return kShapeOk;
}

// ---- the inlier test, float32

// lo2 and hi2 of a record's radius
PCGX_HD void shape_band(float r, float max_dist, float *lo2, float *hi2) {
  const float lo = r - max_dist, hi = r + max_dist;
  *hi2 = hi * hi;
  *lo2 = lo > 0.0f ? lo * lo : -1.0f;
}

// kNormalTest: min_normal_cos != 0, c2 = min_normal_cos * min_normal_cos
template <int kKind, bool kNormalTest>
PCGX_HD bool shape_inlier(const float *rec8, float lo2, float hi2, float c2, float px, float py, float pz, float mx, float my,
                          float mz) {
  const float vx = px - rec8[0], vy = py - rec8[1], vz = pz - rec8[2];
  float d2 = (vx * vx + vy * vy) + vz * vz;
  float g = 0.0f;
  if (kNormalTest) g = (mx * vx + my * vy) + mz * vz;
  if (kKind == kShapeCylinder) {
    const float t = (vx * rec8[4] + vy * rec8[5]) + vz * rec8[6];
    d2 = d2 - t * t;
    if (kNormalTest) g = g - t * ((mx * rec8[4] + my * rec8[5]) + mz * rec8[6]);
  }
  bool in = d2 < hi2 && d2 > lo2;
  if (kNormalTest) in = in && g * g >= c2 * d2;
  return in;
}

PCGX_HD bool shape_inlier_any(int32_t kind, bool normal_test, const float *rec8, float lo2, float hi2, float c2, float px,
                              float py, float pz, float mx, float my, float mz) {
  if (kind == kShapeSphere)
    return normal_test ? shape_inlier<kShapeSphere, true>(rec8, lo2, hi2, c2, px, py, pz, mx, my, mz)
                       : shape_inlier<kShapeSphere, false>(rec8, lo2, hi2, c2, px, py, pz, mx, my, mz);
  return normal_test ? shape_inlier<kShapeCylinder, true>(rec8, lo2, hi2, c2, px, py, pz, mx, my, mz)
                     : shape_inlier<kShapeCylinder, false>(rec8, lo2, hi2, c2, px, py, pz, mx, my, mz);
}

// ---- the refit

// e1 = unit(a x the coordinate axis of a's smallest |component|, the first on a tie), e2 = a x e1
PCGX_HD void shape_cylinder_frame(const double *a, double *e1, double *e2) {
  const double ax = fabs(a[0]), ay = fabs(a[1]), az = fabs(a[2]);
  const int k = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
  const double c[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
  const double x = a[1] * c[2] - a[2] * c[1], y = a[2] * c[0] - a[0] * c[2], z = a[0] * c[1] - a[1] * c[0];
  const double len = sqrt(shape_dot(x, y, z, x, y, z));
  e1[0] = x / len;
  e1[1] = y / len;
  e1[2] = z / len;
  e2[0] = a[1] * e1[2] - a[2] * e1[1];
  e2[1] = a[2] * e1[0] - a[0] * e1[2];
  e2[2] = a[0] * e1[1] - a[1] * e1[0];
}

// the coordinates x of the point p the refit sums over: p - pivot (sphere), ((p - pivot).e1, (p - pivot).e2, 0) (cylinder)
PCGX_HD void shape_refit_coords(int32_t kind, const float *rec8, const float *pf, double *x) {
  const double vx = (double)pf[0] - (double)rec8[0], vy = (double)pf[1] - (double)rec8[1], vz = (double)pf[2] - (double)rec8[2];
  if (kind == kShapeSphere) {
    x[0] = vx;
    x[1] = vy;
    x[2] = vz;
    return;
  }
  const double a[3] = {(double)rec8[4], (double)rec8[5], (double)rec8[6]};
  double e1[3], e2[3];
  shape_cylinder_frame(a, e1, e2);
  x[0] = shape_dot(vx, vy, vz, e1[0], e1[1], e1[2]);
  x[1] = shape_dot(vx, vy, vz, e2[0], e2[1], e2[2]);
  x[2] = 0.0;
}

// one point's terms of the sums
PCGX_HD void shape_refit_terms(const double *x, double *s13) {
  const double q = shape_dot(x[0], x[1], x[2], x[0], x[1], x[2]);
  s13[0] = x[0];
  s13[1] = x[1];
  s13[2] = x[2];
  s13[3] = x[0] * x[0];
  s13[4] = x[0] * x[1];
  s13[5] = x[0] * x[2];
  s13[6] = x[1] * x[1];
  s13[7] = x[1] * x[2];
  s13[8] = x[2] * x[2];
  s13[9] = q * x[0];
  s13[10] = q * x[1];
  s13[11] = q * x[2];
  s13[12] = q;
}

// The refitted record from the sums over n inliers of the record rec8: least squares of |x|^2 - 2 x.u - k over the
// unknowns y = (u, k), rows (2 x, 1): the normal matrix M = [[4 sum x x^T, 2 sum x], [2 sum x^T, n]], the right side
// (2 sum |x|^2 x, sum |x|^2), solved by Cholesky in that order of unknowns.  false (out all zero): no refit.
// (a template so that every loop has constant bounds: the matrices stay in registers on the device)
template <int kKind>
PCGX_HD bool shape_refit_as(const float *rec8, double n, const double *s13, float r_min, float r_max, float *out8) {
  for (int k = 0; k < 8; k++) out8[k] = 0.0f;
  constexpr int32_t kind = kKind;
  constexpr int d = kKind == kShapeSphere ? 3 : 2, m = d + 1;
  double M[4][4], b[4], L[4][4], y[4];
  const int at[3][3] = {{3, 4, 5}, {4, 6, 7}, {5, 7, 8}};
  for (int i = 0; i < d; i++) {
    for (int j = 0; j < d; j++) M[i][j] = 4.0 * s13[at[i][j]];
    M[i][d] = M[d][i] = 2.0 * s13[i];
    b[i] = 2.0 * s13[9 + i];
  }
  M[d][d] = n;
  b[d] = s13[12];
  double big = 0.0;
  for (int i = 0; i < m; i++) big = M[i][i] > big ? M[i][i] : big;
  for (int j = 0; j < m; j++) {
    double piv = M[j][j];
    for (int k = 0; k < j; k++) piv = piv - L[j][k] * L[j][k];
    if (!(piv > 1e-12 * big)) return false;
    L[j][j] = sqrt(piv);
    for (int i = j + 1; i < m; i++) {
      double v = M[i][j];
      for (int k = 0; k < j; k++) v = v - L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  for (int i = 0; i < m; i++) {  // L z = b
    double v = b[i];
    for (int k = 0; k < i; k++) v = v - L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = m - 1; i >= 0; i--) {  // L^T y = z
    double v = y[i];
    for (int k = i + 1; k < m; k++) v = v - L[k][i] * y[k];
    y[i] = v / L[i][i];
  }
  const double u[3] = {y[0], y[1], d == 3 ? y[2] : 0.0};
  const double r2 = y[d] + shape_dot(u[0], u[1], u[2], u[0], u[1], u[2]);
  if (!(r2 > 0.0)) return false;
  const double r = sqrt(r2);
  if (!shape_radius_ok(r, r_min, r_max)) return false;
  double v[8] = {0.0, 0.0, 0.0, r, 0.0, 0.0, 0.0, 0.0};
  if (kind == kShapeSphere) {
    for (int k = 0; k < 3; k++) v[k] = (double)rec8[k] + u[k];
  } else {
    const double a[3] = {(double)rec8[4], (double)rec8[5], (double)rec8[6]};
    double e1[3], e2[3], c[3];
    shape_cylinder_frame(a, e1, e2);
    for (int k = 0; k < 3; k++) c[k] = ((double)rec8[k] + u[0] * e1[k]) + u[1] * e2[k];
    shape_canonical(c, a, v);
    v[4] = a[0];
    v[5] = a[1];
    v[6] = a[2];
  }
  return shape_store(v, out8);
}

PCGX_HD bool shape_refit(int32_t kind, const float *rec8, double n, const double *s13, float r_min, float r_max, float *out8) {
  return kind == kShapeSphere ? shape_refit_as<kShapeSphere>(rec8, n, s13, r_min, r_max, out8)
                              : shape_refit_as<kShapeCylinder>(rec8, n, s13, r_min, r_max, out8);
}

}  // namespace pcgx
