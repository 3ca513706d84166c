// plane_terms.h -- the plane of three points, the tests a hypothesis passes before it gets one, the refitted plane and
// the inlier test, shared by the device kernels (planes.hip) and the host test (tests/cpp/plane_terms_host.cpp): one
// expression, compiled by both.  NOT in the reference: no parity, checked against the NumPy oracle's restatement
// (tests/plane_oracle.py).
//
// Contract (include/pcgx.h, "planes").  Everything but the inlier test is float64 from the float32 points, each
// operation rounded once; build with -ffp-contract=off.
//   sample     the index a random word u names among R points: pose_terms.h's pose_sample_index
//   status     1: two of the three indices are equal; 2: pose_terms.h's pose_triangle_degenerate; 3: the axis test fails
//   plane      e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2, n = c / sqrt((cx cx + cy cy) + cz cz), turned by plane_orient,
//              d = -((nx p0x + ny p0y) + nz p0z); the four numbers rounded once to float32
//   axis test  |(nx ax + ny ay) + nz az| >= (double)min_axis_cos * |a| on the float64 n
//   orient     with an axis: (nx ax + ny ay) + nz az >= 0, and where that is 0 the rule without one; without: the
//              component of largest magnitude is positive, the first such on a tie (group_terms.h's group_sign)
//   inlier     fabsf(((nx px + ny py) + nz pz) + d) < max_dist, all float32; with normals also
//              fabsf((nx mx + ny my) + nz mz) >= min_normal_cos
//   refit      from group geometry's centroid c and axis 2, a: a turned by plane_orient, the axis test, n = float32(a),
//              d = float32(-((ax cx + ay cy) + az cz)); none when the frame is the degenerate one (eig[0] is not > 0)
#pragma once
#include "pose_terms.h"

namespace pcgx {

constexpr int32_t kPlaneNotRun = -1, kPlaneOk = 0, kPlaneBadSample = 1, kPlaneDegenerate = 2, kPlaneAxis = 3;

// The axis constraint of a call: a[3] the axis widened to double, norm = sqrt((ax ax + ay ay) + az az), cos the bound.
struct PlaneAxis {
  int32_t given;
  double a[3], norm, cos;
};

PCGX_HD PlaneAxis plane_axis(const float *axis, float min_axis_cos) {
  PlaneAxis A;
  A.given = axis ? 1 : 0;
  A.a[0] = axis ? (double)axis[0] : 0.0;
  A.a[1] = axis ? (double)axis[1] : 0.0;
  A.a[2] = axis ? (double)axis[2] : 0.0;
  A.norm = sqrt((A.a[0] * A.a[0] + A.a[1] * A.a[1]) + A.a[2] * A.a[2]);
  A.cos = (double)min_axis_cos;
  return A;
}

PCGX_HD bool plane_finite(float v) {
  uint32_t b;
  __builtin_memcpy(&b, &v, 4);
  return (b & 0x7f800000u) != 0x7f800000u;
}
PCGX_HD bool plane_point_live(float x, float y, float z) { return plane_finite(x) && plane_finite(y) && plane_finite(z); }
PCGX_HD bool plane_normal_live(float x, float y, float z) {
  return plane_point_live(x, y, z) && !(x == 0.0f && y == 0.0f && z == 0.0f);
}

PCGX_HD double plane_axis_dot(double x, double y, double z, const PlaneAxis &A) {
  return (x * A.a[0] + y * A.a[1]) + z * A.a[2];
}
PCGX_HD bool plane_axis_ok(double x, double y, double z, const PlaneAxis &A) {
  return !A.given || fabs(plane_axis_dot(x, y, z, A)) >= A.cos * A.norm;
}

PCGX_HD void plane_orient(double &x, double &y, double &z, const PlaneAxis &A) {
  bool flip;
  const double s = A.given ? plane_axis_dot(x, y, z, A) : 0.0;
  if (A.given && s != 0.0) {
    flip = s < 0.0;
  } else {
    const double ax = fabs(x), ay = fabs(y), az = fabs(z);
    const double lead = (ax >= ay && ax >= az) ? x : (ay >= az ? y : z);
    flip = lead < 0.0;
  }
  if (flip) {
    x = -x;
    y = -y;
    z = -z;
  }
}

// The hypothesis of the points p0, p1, p2 at the indices i0, i1, i2: its status, and for kPlaneOk its plane (all zero
// otherwise).
PCGX_HD int32_t plane_hypothesis(uint32_t i0, uint32_t i1, uint32_t i2, const float *p0, const float *p1, const float *p2,
                                 const PlaneAxis &A, float *plane4) {
  plane4[0] = plane4[1] = plane4[2] = plane4[3] = 0.0f;
  if (i0 == i1 || i0 == i2 || i1 == i2) return kPlaneBadSample;
  if (pose_triangle_degenerate(p0, p1, p2)) return kPlaneDegenerate;
  const double ax = (double)p1[0] - (double)p0[0], ay = (double)p1[1] - (double)p0[1], az = (double)p1[2] - (double)p0[2];
  const double bx = (double)p2[0] - (double)p0[0], by = (double)p2[1] - (double)p0[1], bz = (double)p2[2] - (double)p0[2];
  const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const double len = sqrt((cx * cx + cy * cy) + cz * cz);
  double nx = cx / len, ny = cy / len, nz = cz / len;
  if (!plane_axis_ok(nx, ny, nz, A)) return kPlaneAxis;
  plane_orient(nx, ny, nz, A);
  const double d = -((nx * (double)p0[0] + ny * (double)p0[1]) + nz * (double)p0[2]);
  plane4[0] = (float)nx;
  plane4[1] = (float)ny;
  plane4[2] = (float)nz;
  plane4[3] = (float)d;
  return kPlaneOk;
}

// The refitted plane from group geometry's answer for the inlier list; false (plane all zero): no refit
PCGX_HD bool plane_refit(const double *centroid, const double *axis2, double eig0, const PlaneAxis &A, float *plane4) {
  plane4[0] = plane4[1] = plane4[2] = plane4[3] = 0.0f;
  if (!(eig0 > 0.0)) return false;
  double nx = axis2[0], ny = axis2[1], nz = axis2[2];
  if (!plane_axis_ok(nx, ny, nz, A)) return false;
  plane_orient(nx, ny, nz, A);
  const double d = -((nx * centroid[0] + ny * centroid[1]) + nz * centroid[2]);
  plane4[0] = (float)nx;
  plane4[1] = (float)ny;
  plane4[2] = (float)nz;
  plane4[3] = (float)d;
  return true;
}

PCGX_HD bool plane_near(const float *plane4, float px, float py, float pz, float max_dist) {
  return fabsf(((plane4[0] * px + plane4[1] * py) + plane4[2] * pz) + plane4[3]) < max_dist;
}
PCGX_HD bool plane_normal_agrees(const float *plane4, float mx, float my, float mz, float min_normal_cos) {
  return fabsf((plane4[0] * mx + plane4[1] * my) + plane4[2] * mz) >= min_normal_cos;
}

}  // namespace pcgx
