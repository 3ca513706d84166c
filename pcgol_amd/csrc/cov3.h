// cov3.h -- the float64 moments of a neighbourhood and the 3 x 3 eigen-solve of its covariance.
//
// Surface normals (normals.hip) and k-NN covariances (knearest.hip, pcgx_kdtree_covariances) take the same steps:
// NormAcc sums d = p - q in float64 (centred on the query: small cancellation), norm_acc_cov forms
// C = sum d d^T / n - mean mean^T, and norm_acc_solve diagonalises C scaled to unit trace by cyclic Jacobi in double and
// returns the unit eigenvector of the smallest eigenvalue.  Every index is a compile-time constant: A and V stay in
// registers.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace pcgx {

constexpr int kJacobiSweeps = 8;  // upper bound; a sweep that finds nothing to rotate ends the solve

// The moments of one neighbourhood, centred on the query.
struct NormAcc {
  double sx, sy, sz, sxx, sxy, sxz, syy, syz, szz;
  int32_t n;
  float lox, loy, loz, hix, hiy, hiz;  // box of the neighbours: empty box <=> all coincide (or none)

  __device__ __forceinline__ void clear() {
    sx = sy = sz = sxx = sxy = sxz = syy = syz = szz = 0.0;
    n = 0;
    lox = loy = loz = __builtin_inff();
    hix = hiy = hiz = -__builtin_inff();
  }
  __device__ __forceinline__ void add(const float px, const float py, const float pz, const float qx, const float qy,
                                      const float qz) {
    const double dx = (double)px - (double)qx, dy = (double)py - (double)qy, dz = (double)pz - (double)qz;
    sx += dx;
    sy += dy;
    sz += dz;
    sxx = fma(dx, dx, sxx);
    sxy = fma(dx, dy, sxy);
    sxz = fma(dx, dz, sxz);
    syy = fma(dy, dy, syy);
    syz = fma(dy, dz, syz);
    szz = fma(dz, dz, szz);
    n++;
    lox = fminf(lox, px);
    loy = fminf(loy, py);
    loz = fminf(loz, pz);
    hix = fmaxf(hix, px);
    hiy = fmaxf(hiy, py);
    hiz = fmaxf(hiz, pz);
  }
  // the whole wave's partials into every lane (all 64 lanes must be here)
  __device__ __forceinline__ void wave_sum() {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      sx += __shfl_xor(sx, m);
      sy += __shfl_xor(sy, m);
      sz += __shfl_xor(sz, m);
      sxx += __shfl_xor(sxx, m);
      sxy += __shfl_xor(sxy, m);
      sxz += __shfl_xor(sxz, m);
      syy += __shfl_xor(syy, m);
      syz += __shfl_xor(syz, m);
      szz += __shfl_xor(szz, m);
      n += __shfl_xor(n, m);
      lox = fminf(lox, __shfl_xor(lox, m));
      loy = fminf(loy, __shfl_xor(loy, m));
      loz = fminf(loz, __shfl_xor(loz, m));
      hix = fmaxf(hix, __shfl_xor(hix, m));
      hiy = fmaxf(hiy, __shfl_xor(hiy, m));
      hiz = fmaxf(hiz, __shfl_xor(hiz, m));
    }
  }
  __device__ __forceinline__ void merge(const NormAcc &o) {
    sx += o.sx; sy += o.sy; sz += o.sz;
    sxx += o.sxx; sxy += o.sxy; sxz += o.sxz; syy += o.syy; syz += o.syz; szz += o.szz;
    n += o.n;
    lox = fminf(lox, o.lox); loy = fminf(loy, o.loy); loz = fminf(loz, o.loz);
    hix = fmaxf(hix, o.hix); hiy = fmaxf(hiy, o.hiy); hiz = fmaxf(hiz, o.hiz);
  }
};

// One Jacobi rotation in the (p, q) plane of the symmetric A (Numerical Recipes' form); V collects the rotations.
// Every index is a compile-time constant: A and V stay in registers.
template <int p, int q>
__device__ __forceinline__ void jacobi_rotate(double (&A)[3][3], double (&V)[3][3]) {
  constexpr int r = 3 - p - q;
  const double apq = A[p][q];
  if (apq == 0.0) return;
  // (theta^2 overflows for an apq below 1e-154 of the diagonal gap: t = 0, the rotation only drops apq)
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
  const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c;
  A[p][p] -= t * apq;
  A[q][q] += t * apq;
  A[p][q] = A[q][p] = 0.0;
  const double arp = A[r][p], arq = A[r][q];
  A[r][p] = A[p][r] = c * arp - s * arq;
  A[r][q] = A[q][r] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double vkp = V[k][p], vkq = V[k][q];
    V[k][p] = c * vkp - s * vkq;
    V[k][q] = s * vkp + c * vkq;
  }
}

// C = sum d d^T / n - mean mean^T of the a.n >= 1 neighbours into the upper triangle of A
__device__ __forceinline__ void norm_acc_cov(const NormAcc &a, double (&A)[3][3]) {
  const double inv = 1.0 / (double)a.n;
  const double mx = a.sx * inv, my = a.sy * inv, mz = a.sz * inv;
  A[0][0] = a.sxx * inv - mx * mx;
  A[0][1] = a.sxy * inv - mx * my;
  A[0][2] = a.sxz * inv - mx * mz;
  A[1][1] = a.syy * inv - my * my;
  A[1][2] = a.syz * inv - my * mz;
  A[2][2] = a.szz * inv - mz * mz;
}

// The upper triangle of A, trace tr > 0, scaled to unit trace (nothing under- or overflows in the rotations,
// eigenvectors and l0 / sum l unchanged) and diagonalised by cyclic Jacobi (V: the eigenvectors, in columns): e0, e1, e2
// = the scaled eigenvalues, u = the unit eigenvector of the smallest; returns the smallest.
__device__ __forceinline__ double norm_acc_solve(double (&A)[3][3], double (&V)[3][3], const double tr, double &e0,
                                                 double &e1, double &e2, double &ux, double &uy, double &uz) {
  const double sc = 1.0 / tr;
  A[0][0] *= sc; A[0][1] *= sc; A[0][2] *= sc; A[1][1] *= sc; A[1][2] *= sc; A[2][2] *= sc;
  A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
    // an off-diagonal element below 1e-18 of the (unit) trace moves the l0 eigenvector by 1e-18 / (l1 - l0)
    if (fabs(A[0][1]) < 1e-18) A[0][1] = A[1][0] = 0.0;
    if (fabs(A[0][2]) < 1e-18) A[0][2] = A[2][0] = 0.0;
    if (fabs(A[1][2]) < 1e-18) A[1][2] = A[2][1] = 0.0;
    if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
    jacobi_rotate<0, 1>(A, V);
    jacobi_rotate<0, 2>(A, V);
    jacobi_rotate<1, 2>(A, V);
  }
  e0 = A[0][0];
  e1 = A[1][1];
  e2 = A[2][2];
  const int k = (e0 <= e1 && e0 <= e2) ? 0 : (e1 <= e2 ? 1 : 2);
  const double l0 = k == 0 ? e0 : (k == 1 ? e1 : e2);
  ux = k == 0 ? V[0][0] : (k == 1 ? V[0][1] : V[0][2]);
  uy = k == 0 ? V[1][0] : (k == 1 ? V[1][1] : V[1][2]);
  uz = k == 0 ? V[2][0] : (k == 1 ? V[2][1] : V[2][2]);
  const double len = sqrt(ux * ux + uy * uy + uz * uz);
  ux /= len;
  uy /= len;
  uz /= len;
  return l0;
}

// u turned towards the viewpoint v seen from the query q: negated where u . (v - q) < 0 (pcgx_kdtree_normals' rule)
__device__ __forceinline__ void face_viewpoint(double &ux, double &uy, double &uz, const float vx, const float vy,
                                               const float vz, const float qx, const float qy, const float qz) {
  const double dot = ux * ((double)vx - (double)qx) + uy * ((double)vy - (double)qy) + uz * ((double)vz - (double)qz);
  if (dot < 0.0) {
    ux = -ux;
    uy = -uy;
    uz = -uz;
  }
}

}  // namespace pcgx
