// ndt_terms.h -- the arithmetic of the Normal Distributions Transform extension (Biber and Strasser 2003; Magnusson
// 2009; PCL's NormalDistributionsTransform), shared by the device kernels (ndt.hip: ndt_map_kernel, ndt_sums_kernel)
// and the host test (tests/cpp/ndt_terms_host.cpp): one expression, compiled by both.  NOT in the reference: no
// parity, checked against the NumPy oracle's restatement (tests/ndt_oracle.py).
//
// Contract (include/pcgx.h, "Normal Distributions Transform"):
//   voxel   o = origin + v resolution (float64 from the float32 inputs widened), d = p - o per point of the voxel,
//           mean_d = sum d / n, C = (sum d d^T - n mean_d mean_d^T) / (n - 1); invalid: n < max(min_points, 3), all
//           points coincident (the min / max box of normals), trace C <= 0.  Valid: eigenvalues l0 <= l1 <= l2 and
//           eigenvectors V of C (cov3.h's Jacobi solve), l'_k = max(l_k, ratio l2), cov = V diag(l') V^T,
//           icov = V diag(1 / l') V^T, the mean o + mean_d: each rounded to float32 once.
//   pair    q = p - mu, m = q^T M q, w = exp(-k2 m / 2), J_k = e_k, J_{3+k} = e_k x p,
//           e = (2 / k2) (1 - w), g_k = w J_k^T M q, H_kl = w J_k^T M J_l (k <= l); everything float64, mu and M the
//           voxel's float32 mean and icov widened.
//   k2      Magnusson's constants from outlier_ratio and the resolution (ndt_k2): formed on the host in long double and
//           rounded to float64 once, so that the logarithms' cancellations stay below the rounding.
//
// m decides the weight through exp(-k2 m / 2), so an error in m is multiplied by a = k2 m / 2 (hundreds, for a pair a few
// sigma apart), and the plain float64 evaluation of q^T M q errs by roundings of |q|^T |M| |q|, which cancellation in a
// thin voxel's M puts an order of magnitude above m itself.  So m is formed as an unevaluated sum of two float64
// (gicp_terms.h's dd_ helpers: ~2^-104 relative per operation) and rounded to float64 once.  Its inputs are exact:
// M is float32 widened, and q = p - mu, a difference of two float32 in float64, is exact whenever the two exponents are
// within 29 of each other (a coordinate 2^29 times its voxel's mean is not met inside a grid; there q's rounding would
// enter m through sum |q_a (M q)_a|).
//
// Roundings on the longest chain from the inputs to a term, as written (kNdtChain; the tests' bounds use it).  With
// a = k2 m / 2 the weight's argument, u = 2^-53:
//   m: the double-double part counted as ONE rounding (a convention, as in gicp_terms.h) (1); k2 / 2 carries k2's
//   rounding (2); its product with m (3)                                                          -> a:  3 roundings
//   exp: its own error counted as 2 roundings (the device's exp is good to 1 ulp), plus a times its argument's:
//   |dw| <= w (2 + 3 a) u
//   the factor beside w: q (counted as 1 although exact as a rule); M q: product, 2 additions (4);
//   g_{3+k} = J_{3+k} . (M q): product, difference (6); H likewise (<= 4); the product with w (7); so
//   |d(w t)| <= w |t|_abs (2 + 3 a + 7) u <= 9 (1 + a) w |t|_abs u
//   e = (2 / k2) (1 - w): 2 / k2 (2), 1 - w (3), product (4), and dw: <= 9 (2 / k2) ((1 - w) + (1 + a) w) u
//                                                                                                 -> term: 9
// so every term is within kNdtChain u of its sum of absolute values when the weight's share is taken as w (1 + a).
#pragma once
#include "cov3.h"
#include "gicp_terms.h"

namespace pcgx {

constexpr int kNdtChain = 9;

// One more point of a voxel into its moments, centred on the voxel's centre o (float64).
__device__ __forceinline__ void ndt_acc_add(NormAcc &a, const float px, const float py, const float pz, const double ox,
                                            const double oy, const double oz) {
  const double dx = (double)px - ox, dy = (double)py - oy, dz = (double)pz - oz;
  a.sx += dx;
  a.sy += dy;
  a.sz += dz;
  a.sxx = fma(dx, dx, a.sxx);
  a.sxy = fma(dx, dy, a.sxy);
  a.sxz = fma(dx, dz, a.sxz);
  a.syy = fma(dy, dy, a.syy);
  a.syz = fma(dy, dz, a.syz);
  a.szz = fma(dz, dz, a.szz);
  a.n++;
  a.lox = fminf(a.lox, px);
  a.loy = fminf(a.loy, py);
  a.loz = fminf(a.loz, pz);
  a.hix = fmaxf(a.hix, px);
  a.hiy = fmaxf(a.hiy, py);
  a.hiz = fmaxf(a.hiz, pz);
}

// centre of voxel v along one axis
__device__ __forceinline__ double ndt_centre(const float origin, const int64_t v, const float resolution) {
  return (double)origin + (double)v * (double)resolution;
}

struct NdtVoxel {
  float mean[3];
  float cov6[6], icov6[6];  // xx, xy, xz, yy, yz, zz; zero for an invalid voxel
};

// The voxel finish: moments (a.n >= 1 points, centred on o) -> mean, validity, clamped covariance and its inverse.
__device__ __forceinline__ bool ndt_voxel_finish(const NormAcc &a, const double ox, const double oy, const double oz,
                                                 int32_t min_points, const float min_eigen_ratio, NdtVoxel &out) {
  if (min_points < 3) min_points = 3;
  const double n = (double)a.n;
  const double mx = a.sx / n, my = a.sy / n, mz = a.sz / n;
  out.mean[0] = (float)(ox + mx);
  out.mean[1] = (float)(oy + my);
  out.mean[2] = (float)(oz + mz);
#pragma unroll
  for (int k = 0; k < 6; k++) out.cov6[k] = out.icov6[k] = 0.0f;
  const bool spread = !(a.lox == a.hix && a.loy == a.hiy && a.loz == a.hiz);
  if (!(a.n >= min_points && spread)) return false;
  const double inv = 1.0 / (n - 1.0);
  double A[3][3], V[3][3];
  A[0][0] = (a.sxx - (n * mx) * mx) * inv;
  A[0][1] = (a.sxy - (n * mx) * my) * inv;
  A[0][2] = (a.sxz - (n * mx) * mz) * inv;
  A[1][1] = (a.syy - (n * my) * my) * inv;
  A[1][2] = (a.syz - (n * my) * mz) * inv;
  A[2][2] = (a.szz - (n * mz) * mz) * inv;
  const double tr = A[0][0] + A[1][1] + A[2][2];
  if (!(tr > 0.0)) return false;
  double e0, e1, e2, ux, uy, uz;
  norm_acc_solve(A, V, tr, e0, e1, e2, ux, uy, uz);  // (e_k: the eigenvalues over the trace; V: eigenvectors in columns)
  const double emax = fmax(e0, fmax(e1, e2));
  const double floor_e = (double)min_eigen_ratio * emax;
  const double l[3] = {fmax(e0, floor_e) * tr, fmax(e1, floor_e) * tr, fmax(e2, floor_e) * tr};
  const double il[3] = {1.0 / l[0], 1.0 / l[1], 1.0 / l[2]};
  int k = 0;
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = r; c < 3; c++) {
      out.cov6[k] = (float)((l[0] * V[r][0] * V[c][0] + l[1] * V[r][1] * V[c][1]) + l[2] * V[r][2] * V[c][2]);
      out.icov6[k] = (float)((il[0] * V[r][0] * V[c][0] + il[1] * V[r][1] * V[c][1]) + il[2] * V[r][2] * V[c][2]);
      k++;
    }
  return true;
}

// Magnusson's constants (2009, eq. 6.8-6.10, as PCL's ndt.hpp forms them) -> k2; false: outlier_ratio outside (0, 1),
// or k2 not finite or not > 0.  Host only: long double, rounded to float64 once.
inline bool ndt_k2(const float outlier_ratio, const float resolution, double *k2_out) {
  if (!(outlier_ratio > 0.0f && outlier_ratio < 1.0f)) return false;
  const long double o = (long double)outlier_ratio, res = (long double)resolution;
  const long double c1 = 10.0L * (1.0L - o);
  const long double c2 = o / (res * res * res);
  const long double d3 = -logl(c2);
  const long double d1 = -logl(c1 + c2) - d3;
  const long double k2 = -2.0L * logl((-logl(c1 * expl(-0.5L) + c2) - d3) / d1);
  const double r = (double)k2;
  if (!(r > 0.0) || !(r < __builtin_inf())) return false;
  *k2_out = r;
  return true;
}

// One pair's terms: p the moved point, mean / icov6 the voxel's record, half_k2 = k2 / 2, two_over_k2 = 2 / k2.
// -> e, g[6], H[21] (upper triangle row-major), w.
PCGX_HD void ndt_pair_terms(const float px, const float py, const float pz, const float mean[3], const float icov6[6],
                            const double half_k2, const double two_over_k2, double &e, double g[6], double H[21],
                            double &w) {
  const double M[3][3] = {{(double)icov6[0], (double)icov6[1], (double)icov6[2]},
                          {(double)icov6[1], (double)icov6[3], (double)icov6[4]},
                          {(double)icov6[2], (double)icov6[4], (double)icov6[5]}};
  const double x = (double)px, y = (double)py, z = (double)pz;
  const double q[3] = {x - (double)mean[0], y - (double)mean[1], z - (double)mean[2]};
  // t = M q.  Rotation rows J_3 = (0, -z, y), J_4 = (z, 0, -x), J_5 = (-y, x, 0); W[l] = M J_{3+l} (gicp_terms.h's form)
  double t[3], W[3][3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    t[a] = (M[a][0] * q[0] + M[a][1] * q[1]) + M[a][2] * q[2];
    W[0][a] = M[a][2] * y - M[a][1] * z;
    W[1][a] = M[a][0] * z - M[a][2] * x;
    W[2][a] = M[a][1] * x - M[a][0] * y;
  }
  // m = q^T M q as a sum of two float64, rounded once (see the head of the file)
  Dd md{0.0, 0.0};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const Dd ta = dd_add(dd_add(dd_two_prod(M[a][0], q[0]), dd_two_prod(M[a][1], q[1])), dd_two_prod(M[a][2], q[2]));
    md = dd_add(md, dd_mul_d(ta, q[a]));
  }
  const double m = md.h + md.l;
  w = exp(-(half_k2 * m));
  e = two_over_k2 * (1.0 - w);
  g[0] = w * t[0];
  g[1] = w * t[1];
  g[2] = w * t[2];
  g[3] = w * (y * t[2] - z * t[1]);
  g[4] = w * (z * t[0] - x * t[2]);
  g[5] = w * (x * t[1] - y * t[0]);
  int n = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
#pragma unroll
    for (int l = k; l < 3; l++) H[n++] = w * M[k][l];
#pragma unroll
    for (int l = 0; l < 3; l++) H[n++] = w * W[l][k];
  }
  H[n++] = w * (y * W[0][2] - z * W[0][1]);  // J_3 . W[0]
  H[n++] = w * (y * W[1][2] - z * W[1][1]);  // J_3 . W[1]
  H[n++] = w * (y * W[2][2] - z * W[2][1]);  // J_3 . W[2]
  H[n++] = w * (z * W[1][0] - x * W[1][2]);  // J_4 . W[1]
  H[n++] = w * (z * W[2][0] - x * W[2][2]);  // J_4 . W[2]
  H[n++] = w * (x * W[2][1] - y * W[2][0]);  // J_5 . W[2]
}

}  // namespace pcgx
