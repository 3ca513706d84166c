// gicp_terms.h -- one pair's terms of the Generalized ICP extension (Segal, Haehnel, Thrun 2009), shared by the device
// kernel (icp.hip, icp_gicp_sums_kernel) and the host tests (tests/cpp/gicp_terms_host.cpp): one expression, compiled
// by both.  NOT in the reference: no parity, checked against the NumPy oracle's restatement.
//
// Contract (include/pcgx.h, "Generalized ICP"): with p the re-projected target (float32), b its partner, C_b / C_t
// their covariances, R the upper-left 3 x 3 of the session's pose, from the float32 inputs widened:
//   r = p - b,  S = C_b + R C_t R^T,  M = S^-1 (held fixed within an iteration),
//   J_k = e_k, J_{3+k} = e_k x p  (p' = p + t + w x p, parameters {t, w} as pcgx_math.h),
//   e = r^T M r,  g_k = J_k^T M r,  H_kl = J_k^T M J_l (k <= l, row-major upper triangle).
// Drop rule (gauss_newton_solve's): trace(S) > 0 and every pivot of the float64 Cholesky factorisation of S (rounded
// to float64) > 1e-12 trace(S), else the pair is not used -- false is returned and nothing is written.  NaN anywhere
// in S fails one of the comparisons by itself.
//
// M's entries are formed to a few float64 roundings EACH, however much cancels inside them: an off-diagonal entry of
// S^-1 is a difference of products of S's entries and can come out far below their scale (H_01 = M_01 is such a
// term on its own), and one float64 rounding of S already moves it by 2^-53 (|M| |S| |M|)_kl, which no multiple of
// cond(S) |M_kl| bounds.  So S, its adjugate and its determinant are carried as unevaluated sums of two float64
// (error-free two_sum / two_prod with fma: ~2^-104 relative per operation) and rounded to float64 once, at the
// quotient.  The terms are then plain float64 sums of products of M, J and r.
//
// Roundings on the longest chain from the inputs to a term, as written (kGicpChain; the tests' bounds use it):
//   the double-double part (S, adjugate, determinant; ~2^-104 relative per operation) counted as ONE rounding -- a
//   convention, not a count: change the dd_ helpers or add dd operations and this line is to be looked at again (1);
//   adj, det -> float64 (side by side: 2); their quotient (3)                                            -> M:     3
//   M r: product, 2 additions (6); r itself is 1 rounding, on a shorter chain; M J_{3+l}: product, difference (5)
//   e = r . (M r): product, 2 additions (9); g_{3+k} = J_{3+k} . (M r): product, difference (8); H likewise (<= 7)
//                                                                                                        -> term:  9
#pragma once
#include "pcgx_math.h"

namespace pcgx {

constexpr int kGicpChain = 9;

struct Dd {  // hi + lo, |lo| <= ulp(hi) / 2
  double h, l;
};
PCGX_HD Dd dd_renorm(double s, double e) {
  const double h = s + e;
  return Dd{h, e - (h - s)};
}
PCGX_HD Dd dd_two_prod(double a, double b) {
  const double p = a * b;
  return Dd{p, fma(a, b, -p)};
}
PCGX_HD Dd dd_add(const Dd &x, const Dd &y) {
  const double s = x.h + y.h, bb = s - x.h;
  const double e = ((x.h - (s - bb)) + (y.h - bb)) + (x.l + y.l);
  return dd_renorm(s, e);
}
PCGX_HD Dd dd_neg(const Dd &x) { return Dd{-x.h, -x.l}; }
PCGX_HD Dd dd_mul_d(const Dd &x, double d) {
  const Dd p = dd_two_prod(x.h, d);
  return dd_renorm(p.h, p.l + x.l * d);
}
PCGX_HD Dd dd_mul(const Dd &x, const Dd &y) {
  const Dd p = dd_two_prod(x.h, y.h);
  return dd_renorm(p.h, p.l + (x.h * y.l + x.l * y.h));
}

// p, b: the pair; cb, ct: xx, xy, xz, yy, yz, zz; m: the pose (column-major Mat4, only its rotation block is read).
PCGX_HD bool gicp_terms(float px, float py, float pz, float bx, float by, float bz, const float cb[6],
                        const float ct[6], const float *m, double &e, double g[6], double H[21]) {
  const double R[3][3] = {{(double)m[0], (double)m[4], (double)m[8]},
                          {(double)m[1], (double)m[5], (double)m[9]},
                          {(double)m[2], (double)m[6], (double)m[10]}};
  const double C[3][3] = {{(double)ct[0], (double)ct[1], (double)ct[2]},
                          {(double)ct[1], (double)ct[3], (double)ct[4]},
                          {(double)ct[2], (double)ct[4], (double)ct[5]}};
  Dd A[3][3];  // R C_t (a product of two float32 is exact in float64)
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double p0 = R[a][0] * C[0][k], p1 = R[a][1] * C[1][k], p2 = R[a][2] * C[2][k];
      A[a][k] = dd_add(dd_add(Dd{p0, 0.0}, Dd{p1, 0.0}), Dd{p2, 0.0});
    }
  // S, lower triangle, index (a, b) -> a (a + 1) / 2 + b: s00, s10, s11, s20, s21, s22
  Dd S[6];
  const double cbl[6] = {(double)cb[0], (double)cb[1], (double)cb[3], (double)cb[2], (double)cb[4], (double)cb[5]};
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b <= a; b++) {
      const Dd t = dd_add(dd_add(dd_mul_d(A[a][0], R[b][0]), dd_mul_d(A[a][1], R[b][1])), dd_mul_d(A[a][2], R[b][2]));
      S[a * (a + 1) / 2 + b] = dd_add(t, Dd{cbl[a * (a + 1) / 2 + b], 0.0});
    }
  const Dd &S00 = S[0], &S10 = S[1], &S11 = S[2], &S20 = S[3], &S21 = S[4], &S22 = S[5];
  {  // the drop rule, on S rounded to float64
    const double s00 = S00.h, s10 = S10.h, s11 = S11.h, s20 = S20.h, s21 = S21.h, s22 = S22.h;
    const double tr = (s00 + s11) + s22;
    if (!(tr > 0.0)) return false;
    const double tiny = tr * 1e-12;
    if (!(s00 > tiny)) return false;
    const double l00 = sqrt(s00);
    const double l10 = s10 / l00, l20 = s20 / l00;
    const double d1 = s11 - l10 * l10;
    if (!(d1 > tiny)) return false;
    const double l11 = sqrt(d1);
    const double l21 = (s21 - l20 * l10) / l11;
    const double d2 = (s22 - l20 * l20) - l21 * l21;
    if (!(d2 > tiny)) return false;
  }
  // adjugate (symmetric) and determinant
  const Dd a00 = dd_add(dd_mul(S11, S22), dd_neg(dd_mul(S21, S21)));
  const Dd a01 = dd_add(dd_mul(S20, S21), dd_neg(dd_mul(S10, S22)));
  const Dd a02 = dd_add(dd_mul(S10, S21), dd_neg(dd_mul(S20, S11)));
  const Dd a11 = dd_add(dd_mul(S00, S22), dd_neg(dd_mul(S20, S20)));
  const Dd a12 = dd_add(dd_mul(S10, S20), dd_neg(dd_mul(S00, S21)));
  const Dd a22 = dd_add(dd_mul(S00, S11), dd_neg(dd_mul(S10, S10)));
  const Dd det = dd_add(dd_add(dd_mul(S00, a00), dd_mul(S10, a01)), dd_mul(S20, a02));
  const double dt = det.h + det.l;
  const double M[3][3] = {{(a00.h + a00.l) / dt, (a01.h + a01.l) / dt, (a02.h + a02.l) / dt},
                          {(a01.h + a01.l) / dt, (a11.h + a11.l) / dt, (a12.h + a12.l) / dt},
                          {(a02.h + a02.l) / dt, (a12.h + a12.l) / dt, (a22.h + a22.l) / dt}};
  const double x = (double)px, y = (double)py, z = (double)pz;
  const double r[3] = {x - (double)bx, y - (double)by, z - (double)bz};
  // w = M r.  Translation rows (J_k = e_k): g_k = w_k and H_kl = M_kl as they stand.  Rotation rows: J_3 = (0, -z, y),
  // J_4 = (z, 0, -x), J_5 = (-y, x, 0) have two non-zero entries each; W[l] = M J_{3+l}.
  double w[3], W[3][3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    w[a] = (M[a][0] * r[0] + M[a][1] * r[1]) + M[a][2] * r[2];
    W[0][a] = M[a][2] * y - M[a][1] * z;
    W[1][a] = M[a][0] * z - M[a][2] * x;
    W[2][a] = M[a][1] * x - M[a][0] * y;
  }
  e = (r[0] * w[0] + r[1] * w[1]) + r[2] * w[2];
  g[0] = w[0];
  g[1] = w[1];
  g[2] = w[2];
  g[3] = y * w[2] - z * w[1];
  g[4] = z * w[0] - x * w[2];
  g[5] = x * w[1] - y * w[0];
  // H, upper triangle row-major: rows 0..2 = {M_k., W[.][k]}, rows 3..5 = J_{3+k} . W[l]
  int n = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
#pragma unroll
    for (int l = k; l < 3; l++) H[n++] = M[k][l];
#pragma unroll
    for (int l = 0; l < 3; l++) H[n++] = W[l][k];
  }
  H[n++] = y * W[0][2] - z * W[0][1];  // J_3 . W[0]
  H[n++] = y * W[1][2] - z * W[1][1];  // J_3 . W[1]
  H[n++] = y * W[2][2] - z * W[2][1];  // J_3 . W[2]
  H[n++] = z * W[1][0] - x * W[1][2];  // J_4 . W[1]
  H[n++] = z * W[2][0] - x * W[2][2];  // J_4 . W[2]
  H[n++] = x * W[2][1] - y * W[2][0];  // J_5 . W[2]
  return true;
}

}  // namespace pcgx
