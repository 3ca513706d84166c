// pose_terms.h -- the rigid pose of a set of point pairs, and the tests a three-pair hypothesis passes before it gets
// one, shared by the device kernels (pose.hip) and the host test (tests/cpp/pose_terms_host.cpp): one expression,
// compiled by both.  NOT in the reference: no parity, checked against the NumPy oracle's restatement
// (tests/pose_oracle.py), whose rigid solve is another method (Kabsch by SVD).
//
// Contract (include/pcgx.h, "pose from correspondences").  Everything but the inlier test is float64 from the float32
// points; build with -ffp-contract=off.
//   sample     the index a random word u names among m pairs: (uint64(u) * m) >> 32
//   triangle   degenerate when !(|e1 x e2|^2 > 1e-12 |e1|^2 |e2|^2), e1 = x1 - x0, e2 = x2 - x0 (a NaN is degenerate)
//   edges      ls, ld the lengths of one edge in the source and in the target: the hypothesis is dropped when
//              !(ls >= s ld) or !(ld >= s ls) for one of the three edges
//   solve      the proper rotation R and the translation t that minimise sum |R p + t - q|^2, from the moments
//              {n, sum p, sum q, sum p q^T} taken about an origin pair (op, oq): Horn's unit quaternion, the eigenvector
//              of the largest eigenvalue of his symmetric 4 x 4 matrix N, by cyclic Jacobi in double (cov3.h's rotation
//              with four rows).  It cannot return a reflection.  The three-pair hypothesis and the refit over an inlier
//              set are this one function.  It also returns the two largest eigenvalues l1 >= l2 of N scaled to a unit
//              largest moment: l1 - l2 is what fixes the rotation about the best axis, and the refit's degeneracy rule.
//   inlier     x' = mat4_transform(pose, p), d = q - x', (dx dx + dy dy) + dz dz < max_dist_sq, all float32
#pragma once
#include "pcgx_math.h"

namespace pcgx {

constexpr int32_t kPoseOk = 0, kPoseBadSample = 1, kPoseDegenerate = 2, kPoseEdge = 3;
constexpr double kPoseTriangleEps = 1e-12;  // on sin^2 of the angle between two edges
constexpr double kPoseRefitGap = 1e-9;      // an inlier set is refitted when n >= 3 and l1 - l2 > this * l1
constexpr int kPoseJacobiSweeps = 12;       // upper bound; a sweep that finds nothing to rotate ends the solve

PCGX_HD uint32_t pose_sample_index(uint32_t u, uint32_t m) { return (uint32_t)(((uint64_t)u * (uint64_t)m) >> 32); }

PCGX_HD bool pose_triangle_degenerate(const float *x0, const float *x1, const float *x2) {
  const double ax = (double)x1[0] - (double)x0[0], ay = (double)x1[1] - (double)x0[1], az = (double)x1[2] - (double)x0[2];
  const double bx = (double)x2[0] - (double)x0[0], by = (double)x2[1] - (double)x0[1], bz = (double)x2[2] - (double)x0[2];
  const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const double c2 = (cx * cx + cy * cy) + cz * cz;
  const double a2 = (ax * ax + ay * ay) + az * az, b2 = (bx * bx + by * by) + bz * bz;
  return !(c2 > (kPoseTriangleEps * a2) * b2);
}

PCGX_HD double pose_edge_len(const float *a, const float *b) {
  const double x = (double)b[0] - (double)a[0], y = (double)b[1] - (double)a[1], z = (double)b[2] - (double)a[2];
  return sqrt((x * x + y * y) + z * z);
}

// true when one of the three edges is too different in the two triangles; s in (0, 1]
PCGX_HD bool pose_edges_differ(const float *p0, const float *p1, const float *p2, const float *q0, const float *q1,
                               const float *q2, double s) {
  const double l0 = pose_edge_len(p0, p1), d0 = pose_edge_len(q0, q1);
  const double l1 = pose_edge_len(p0, p2), d1 = pose_edge_len(q0, q2);
  const double l2 = pose_edge_len(p1, p2), d2 = pose_edge_len(q1, q2);
  const bool ok = l0 >= s * d0 && d0 >= s * l0 && l1 >= s * d1 && d1 >= s * l1 && l2 >= s * d2 && d2 >= s * l2;
  return !ok;
}

// The moments of pairs (p, q) about the origin pair (op, oq).
struct PoseMoments {
  double n, sp[3], sq[3], spq[3][3];  // spq[a][b] = sum (p - op)_a (q - oq)_b
};

PCGX_HD void pose_moments_clear(PoseMoments &a) {
  a.n = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    a.sp[i] = a.sq[i] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) a.spq[i][j] = 0.0;
  }
}

PCGX_HD void pose_moments_add(PoseMoments &a, const float *p, const float *q, const float *op, const float *oq) {
  const double dp[3] = {(double)p[0] - (double)op[0], (double)p[1] - (double)op[1], (double)p[2] - (double)op[2]};
  const double dq[3] = {(double)q[0] - (double)oq[0], (double)q[1] - (double)oq[1], (double)q[2] - (double)oq[2]};
  a.n += 1.0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    a.sp[i] += dp[i];
    a.sq[i] += dq[i];
#pragma unroll
    for (int j = 0; j < 3; j++) a.spq[i][j] += dp[i] * dq[j];
  }
}

PCGX_HD void pose_moments_merge(PoseMoments &a, const PoseMoments &o) {
  a.n += o.n;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    a.sp[i] += o.sp[i];
    a.sq[i] += o.sq[i];
#pragma unroll
    for (int j = 0; j < 3; j++) a.spq[i][j] += o.spq[i][j];
  }
}

// cov3.h's jacobi_rotate with four rows: one rotation in the (p, q) plane of the symmetric A; V collects the
// rotations.  Every index is a compile-time constant once the loops are unrolled: A and V stay in registers.
template <int p, int q>
PCGX_HD void pose_jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[p][q];
  if (apq == 0.0) return;
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
  const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c;
  A[p][p] -= t * apq;
  A[q][q] += t * apq;
  A[p][q] = A[q][p] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    if (r == p || r == q) continue;
    const double arp = A[r][p], arq = A[r][q];
    A[r][p] = A[p][r] = c * arp - s * arq;
    A[r][q] = A[q][r] = s * arp + c * arq;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double vkp = V[k][p], vkq = V[k][q];
    V[k][p] = c * vkp - s * vkq;
    V[k][q] = s * vkp + c * vkq;
  }
}

// The pose of the moments a (a.n >= 1) about (op, oq) into the column-major pose16, each of the twelve numbers rounded
// once to float32, the bottom row 0 0 0 1.  l1 >= l2: the two largest eigenvalues of N over the largest |moment|.
// false (pose16 all zero, l1 = l2 = 0) when the centred sum p q^T is zero or not finite: nothing fixes a rotation.
PCGX_HD bool pose_solve(const PoseMoments &a, const float *op, const float *oq, float *pose16, double &l1, double &l2) {
  for (int i = 0; i < 16; i++) pose16[i] = 0.0f;
  l1 = l2 = 0.0;
  const double inv = 1.0 / a.n;
  double S[3][3], big = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      S[i][j] = a.spq[i][j] - (a.sp[i] * a.sq[j]) * inv;
      big = fmax(big, fabs(S[i][j]));  // (fmax drops a NaN: the test below is on the sum)
    }
  const double sum = ((S[0][0] + S[0][1]) + (S[0][2] + S[1][0])) + ((S[1][1] + S[1][2]) + (S[2][0] + S[2][1])) + S[2][2];
  if (!(big > 0.0) || !(fabs(sum) < __builtin_inf()) || !(big < __builtin_inf())) return false;
  const double sc = 1.0 / big;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) S[i][j] *= sc;
  double A[4][4], V[4][4];
  A[0][0] = (S[0][0] + S[1][1]) + S[2][2];
  A[1][1] = (S[0][0] - S[1][1]) - S[2][2];
  A[2][2] = (S[1][1] - S[0][0]) - S[2][2];
  A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
  A[0][1] = A[1][0] = S[1][2] - S[2][1];
  A[0][2] = A[2][0] = S[2][0] - S[0][2];
  A[0][3] = A[3][0] = S[0][1] - S[1][0];
  A[1][2] = A[2][1] = S[0][1] + S[1][0];
  A[1][3] = A[3][1] = S[2][0] + S[0][2];
  A[2][3] = A[3][2] = S[1][2] + S[2][1];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kPoseJacobiSweeps; sweep++) {
    // (the entries of N are at most 3 in size: an off-diagonal element below 1e-18 moves nothing a double can hold)
    bool any = false;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = r + 1; c < 4; c++) {
        if (fabs(A[r][c]) < 1e-18) A[r][c] = A[c][r] = 0.0;
        any = any || A[r][c] != 0.0;
      }
    if (!any) break;
    pose_jacobi_rotate<0, 1>(A, V);
    pose_jacobi_rotate<0, 2>(A, V);
    pose_jacobi_rotate<0, 3>(A, V);
    pose_jacobi_rotate<1, 2>(A, V);
    pose_jacobi_rotate<1, 3>(A, V);
    pose_jacobi_rotate<2, 3>(A, V);
  }
  const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2], e3 = A[3][3];
  const int k = (e0 >= e1 && e0 >= e2 && e0 >= e3) ? 0 : ((e1 >= e2 && e1 >= e3) ? 1 : (e2 >= e3 ? 2 : 3));
  l1 = k == 0 ? e0 : (k == 1 ? e1 : (k == 2 ? e2 : e3));
  const double ninf = -__builtin_inf();
  l2 = fmax(fmax(k == 0 ? ninf : e0, k == 1 ? ninf : e1), fmax(k == 2 ? ninf : e2, k == 3 ? ninf : e3));
  double qw = k == 0 ? V[0][0] : (k == 1 ? V[0][1] : (k == 2 ? V[0][2] : V[0][3]));
  double qx = k == 0 ? V[1][0] : (k == 1 ? V[1][1] : (k == 2 ? V[1][2] : V[1][3]));
  double qy = k == 0 ? V[2][0] : (k == 1 ? V[2][1] : (k == 2 ? V[2][2] : V[2][3]));
  double qz = k == 0 ? V[3][0] : (k == 1 ? V[3][1] : (k == 2 ? V[3][2] : V[3][3]));
  const double len = sqrt((qw * qw + qx * qx) + (qy * qy + qz * qz));
  qw /= len;
  qx /= len;
  qy /= len;
  qz /= len;
  double R[3][3];
  R[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz);
  R[0][1] = 2.0 * (qx * qy - qw * qz);
  R[0][2] = 2.0 * (qx * qz + qw * qy);
  R[1][0] = 2.0 * (qx * qy + qw * qz);
  R[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz);
  R[1][2] = 2.0 * (qy * qz - qw * qx);
  R[2][0] = 2.0 * (qx * qz - qw * qy);
  R[2][1] = 2.0 * (qy * qz + qw * qx);
  R[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
  const double cp[3] = {(double)op[0] + a.sp[0] * inv, (double)op[1] + a.sp[1] * inv, (double)op[2] + a.sp[2] * inv};
  const double cq[3] = {(double)oq[0] + a.sq[0] * inv, (double)oq[1] + a.sq[1] * inv, (double)oq[2] + a.sq[2] * inv};
#pragma unroll
  for (int r = 0; r < 3; r++) {
    pose16[r] = (float)R[r][0];
    pose16[4 + r] = (float)R[r][1];
    pose16[8 + r] = (float)R[r][2];
    pose16[12 + r] = (float)(cq[r] - ((R[r][0] * cp[0] + R[r][1] * cp[1]) + R[r][2] * cp[2]));
  }
  pose16[15] = 1.0f;
  return true;
}

// may an inlier set with these moments be refitted?  (the header's rule: at least three pairs, not all on a line)
PCGX_HD bool pose_refit_allowed(double n, bool solved, double l1, double l2) {
  return solved && n >= 3.0 && (l1 - l2) > kPoseRefitGap * l1;
}

// Hypothesis from the three samples u[0..2] over m pairs: its status, and for kPoseOk its pose (all zero otherwise).
PCGX_HD int32_t pose_hypothesis(const float *src_xyz, int64_t ns, const float *dst_xyz, int64_t nd,
                                const int32_t *src_ids, const int32_t *dst_ids, int64_t m, const uint32_t *u,
                                float edge_similarity, float *pose16) {
  for (int i = 0; i < 16; i++) pose16[i] = 0.0f;
  if (m < 3) return kPoseBadSample;
  const uint32_t i0 = pose_sample_index(u[0], (uint32_t)m), i1 = pose_sample_index(u[1], (uint32_t)m),
                 i2 = pose_sample_index(u[2], (uint32_t)m);
  if (i0 == i1 || i0 == i2 || i1 == i2) return kPoseBadSample;
  const int64_t s0 = src_ids[i0], s1 = src_ids[i1], s2 = src_ids[i2];
  const int64_t d0 = dst_ids[i0], d1 = dst_ids[i1], d2 = dst_ids[i2];
  if (s0 < 0 || s0 >= ns || s1 < 0 || s1 >= ns || s2 < 0 || s2 >= ns) return kPoseBadSample;
  if (d0 < 0 || d0 >= nd || d1 < 0 || d1 >= nd || d2 < 0 || d2 >= nd) return kPoseBadSample;
  const float *p0 = src_xyz + 3 * s0, *p1 = src_xyz + 3 * s1, *p2 = src_xyz + 3 * s2;
  const float *q0 = dst_xyz + 3 * d0, *q1 = dst_xyz + 3 * d1, *q2 = dst_xyz + 3 * d2;
  if (pose_triangle_degenerate(p0, p1, p2) || pose_triangle_degenerate(q0, q1, q2)) return kPoseDegenerate;
  if (edge_similarity > 0.0f && pose_edges_differ(p0, p1, p2, q0, q1, q2, (double)edge_similarity)) return kPoseEdge;
  PoseMoments a;
  pose_moments_clear(a);
  pose_moments_add(a, p0, q0, p0, q0);
  pose_moments_add(a, p1, q1, p0, q0);
  pose_moments_add(a, p2, q2, p0, q0);
  double l1, l2;
  if (!pose_solve(a, p0, q0, pose16, l1, l2)) return kPoseDegenerate;  // (two non-degenerate triangles: never)
  return kPoseOk;
}

// DistSq of pair (p, q) under the pose, the expressions of the ICP kernels; the pair is an inlier when it is
// < max_dist_sq (false for a NaN)
PCGX_HD float pose_dist_sq(const float *pose16, const float *p, const float *q) {
  float x, y, z;
  mat4_transform(pose16, p[0], p[1], p[2], x, y, z);
  const float dx = q[0] - x, dy = q[1] - y, dz = q[2] - z;
  return (dx * dx + dy * dy) + dz * dz;
}

}  // namespace pcgx
