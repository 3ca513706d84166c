// mls_terms.h -- the arithmetic of moving-least-squares smoothing (Alexa et al. 2003; PCL's MovingLeastSquares with the
// SIMPLE projection), shared by the device kernel (mls.hip, mls_kernel) and the host test
// (tests/cpp/mls_terms_host.cpp): one expression, compiled by both.  NOT in the reference: no parity, checked against
// the NumPy oracle's restatement (tests/mls_oracle.py).
//
// Contract (include/pcgx.h, "moving least squares"): for a query q with neighbours p, d = p - q in float64,
//   frame: C, mean as normals have them (NormAcc, norm_acc_cov, norm_acc_solve); n = unit eigenvector of the smallest
//          eigenvalue, u, v the other two; d0 = (mean . n) n: the query's projection onto the plane through the
//          centroid.  No frame (kind 0): fewer than min_nb neighbours, all coincident, trace of C <= 0.
//   plane (kind 1): q + d0, normal n.
//   polynomial (kind 2; order 2 and count >= 6): per neighbour e = d - d0, h = e . n, a = (e . u) / radius,
//          b = (e . v) / radius, w = exp(-|e|^2 / sigma^2), B = (1, a, b, a^2, a b, b^2); M = sum w B B^T,
//          g = sum w B h (MlsAcc); c = M^-1 g by Cholesky in the basis' order, which fails when sum w is not > 0 or a
//          pivot s_k = M_kk - sum_j L_kj^2 is not above 1e-10 M_kk; a failed solve, or |c0| > radius, is kind 1; else
//          q + d0 + c0 n, normal n - (c1 / radius) u - (c2 / radius) v, normalised.
//   Normals of kind 1 and 2 are turned towards the viewpoint (face_viewpoint); positions and normals are rounded to
//   float32 once.  Which u, v the eigen-solve returns does not move the result (the basis spans every polynomial of
//   degree <= 2 and w depends on |e| only); it moves the pivots, so a solve near the threshold may go either way.
// Every index is a compile-time constant after unrolling: the 28 sums, L and c stay in registers.
#pragma once
#include "cov3.h"

namespace pcgx {

enum { kMlsUnchanged = 0, kMlsPlane = 1, kMlsPoly = 2 };  // PCGX_MLS_* (include/pcgx.h)

constexpr int kMlsBasis = 6;                                // 1, a, b, a^2, a b, b^2
constexpr int kMlsTri = kMlsBasis * (kMlsBasis + 1) / 2;    // upper triangle of M, row-major
constexpr double kMlsPivotMin = 1e-10;                      // a pivot must exceed this share of its diagonal element

// place of M[i][j], i <= j, in the row-major upper triangle
constexpr int mls_tri(const int i, const int j) { return i * kMlsBasis - i * (i - 1) / 2 + (j - i); }

// The local frame of one query: the reference plane and its in-plane axes, and the two scales.
struct MlsFrame {
  double nx, ny, nz, ux, uy, uz, vx, vy, vz;
  double d0x, d0y, d0z;  // q + d0: the query's projection onto the plane through the centroid
  double inv_r, inv_s2;  // 1 / radius, 1 / sigma^2
};

// The frame of the neighbourhood `a` (pass 1's moments); false: no plane can be fitted (kind 0), F is not written.
__device__ __forceinline__ bool mls_frame(const NormAcc &a, const int32_t min_nb, const float radius, const float sigma,
                                          MlsFrame &F) {
  const bool spread = !(a.lox == a.hix && a.loy == a.hiy && a.loz == a.hiz);
  if (!(a.n >= min_nb && spread)) return false;
  double A[3][3], V[3][3];
  norm_acc_cov(a, A);
  const double tr = A[0][0] + A[1][1] + A[2][2];
  if (!(tr > 0.0)) return false;
  double e0, e1, e2;
  norm_acc_solve(A, V, tr, e0, e1, e2, F.nx, F.ny, F.nz);
  // u: the column after the smallest eigenvalue's (norm_acc_solve's choice of k, restated), made unit; v = n x u
  const int k = (e0 <= e1 && e0 <= e2) ? 0 : (e1 <= e2 ? 1 : 2);
  double ux = k == 0 ? V[0][1] : (k == 1 ? V[0][2] : V[0][0]);
  double uy = k == 0 ? V[1][1] : (k == 1 ? V[1][2] : V[1][0]);
  double uz = k == 0 ? V[2][1] : (k == 1 ? V[2][2] : V[2][0]);
  const double ul = sqrt(ux * ux + uy * uy + uz * uz);
  ux /= ul; uy /= ul; uz /= ul;
  double vx = F.ny * uz - F.nz * uy, vy = F.nz * ux - F.nx * uz, vz = F.nx * uy - F.ny * ux;
  const double vl = sqrt(vx * vx + vy * vy + vz * vz);
  F.ux = ux; F.uy = uy; F.uz = uz;
  F.vx = vx / vl; F.vy = vy / vl; F.vz = vz / vl;
  const double inv = 1.0 / (double)a.n;
  const double t = (a.sx * inv) * F.nx + (a.sy * inv) * F.ny + (a.sz * inv) * F.nz;
  F.d0x = t * F.nx; F.d0y = t * F.ny; F.d0z = t * F.nz;
  F.inv_r = 1.0 / (double)radius;
  F.inv_s2 = 1.0 / ((double)sigma * (double)sigma);
  return true;
}

// The weighted normal equations of one neighbourhood: M's upper triangle, g, sum w.
struct MlsAcc {
  double m[kMlsTri], g[kMlsBasis], sw;

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < kMlsTri; k++) m[k] = 0.0;
#pragma unroll
    for (int k = 0; k < kMlsBasis; k++) g[k] = 0.0;
    sw = 0.0;
  }
  __device__ __forceinline__ void add(const float px, const float py, const float pz, const float qx, const float qy,
                                      const float qz, const MlsFrame &F) {
    const double ex = ((double)px - (double)qx) - F.d0x, ey = ((double)py - (double)qy) - F.d0y,
                 ez = ((double)pz - (double)qz) - F.d0z;
    const double h = ex * F.nx + ey * F.ny + ez * F.nz;
    const double a = (ex * F.ux + ey * F.uy + ez * F.uz) * F.inv_r, b = (ex * F.vx + ey * F.vy + ez * F.vz) * F.inv_r;
    const double w = exp(-(ex * ex + ey * ey + ez * ez) * F.inv_s2);
    const double B[kMlsBasis] = {1.0, a, b, a * a, a * b, b * b};
#pragma unroll
    for (int i = 0; i < kMlsBasis; i++) {
      const double wb = w * B[i];
#pragma unroll
      for (int j = i; j < kMlsBasis; j++) m[mls_tri(i, j)] = fma(wb, B[j], m[mls_tri(i, j)]);
      g[i] = fma(wb, h, g[i]);
    }
    sw += w;
  }
  // the whole wave's partials into every lane (all 64 lanes must be here)
  __device__ __forceinline__ void wave_sum() {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
      for (int k = 0; k < kMlsTri; k++) m[k] += __shfl_xor(m[k], s);
#pragma unroll
      for (int k = 0; k < kMlsBasis; k++) g[k] += __shfl_xor(g[k], s);
      sw += __shfl_xor(sw, s);
    }
  }
  __device__ __forceinline__ void merge(const MlsAcc &o) {
#pragma unroll
    for (int k = 0; k < kMlsTri; k++) m[k] += o.m[k];
#pragma unroll
    for (int k = 0; k < kMlsBasis; k++) g[k] += o.g[k];
    sw += o.sw;
  }
};

// c = M^-1 g by Cholesky (M = L L^T, pivots in the basis' order) and two substitutions.  false: sum w is not > 0, or
// a pivot is not above kMlsPivotMin of its diagonal element.  pivot_ratio: the smallest s_k / M_kk met (0 where sum w
// or a diagonal element is not > 0): how far the solve was from failing, or by how much it failed.
__device__ __forceinline__ bool mls_solve(const MlsAcc &a, double (&c)[kMlsBasis], double &pivot_ratio) {
  pivot_ratio = 0.0;
  if (!(a.sw > 0.0)) return false;
  double L[kMlsBasis][kMlsBasis];
  double ratio = 1.0;
#pragma unroll
  for (int j = 0; j < kMlsBasis; j++) {
    const double mjj = a.m[mls_tri(j, j)];
    double s = mjj;
#pragma unroll
    for (int k = 0; k < j; k++) s -= L[j][k] * L[j][k];
    if (!(mjj > 0.0)) return false;
    ratio = fmin(ratio, s / mjj);
    pivot_ratio = ratio;
    if (!(s > kMlsPivotMin * mjj)) return false;
    const double l = sqrt(s);
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < kMlsBasis; i++) {
      double t = a.m[mls_tri(j, i)];
#pragma unroll
      for (int k = 0; k < j; k++) t -= L[i][k] * L[j][k];
      L[i][j] = t / l;
    }
  }
  double y[kMlsBasis];
#pragma unroll
  for (int i = 0; i < kMlsBasis; i++) {  // L y = g
    double t = a.g[i];
#pragma unroll
    for (int k = 0; k < i; k++) t -= L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = kMlsBasis - 1; i >= 0; i--) {  // L^T c = y
    double t = y[i];
#pragma unroll
    for (int k = i + 1; k < kMlsBasis; k++) t -= L[k][i] * c[k];
    c[i] = t / L[i][i];
  }
  return true;
}

// One query's answer (the contract in the file's head).
struct MlsResult {
  int32_t kind;
  float px, py, pz, nx, ny, nz;
  double pivot_ratio, c0;  // of the polynomial solve (0 where none was tried): what the tests' bands are made of
};

// framed: mls_frame's answer, F its frame; poly: the equations in `a` were summed (order 2, count >= 6).
__device__ __forceinline__ MlsResult mls_finish(const bool framed, const MlsFrame &F, const bool poly, const MlsAcc &a,
                                                const float radius, const float qx, const float qy, const float qz,
                                                const float vx, const float vy, const float vz) {
  MlsResult R;
  R.kind = kMlsUnchanged;
  R.px = qx; R.py = qy; R.pz = qz;  // the query's own bits
  R.nx = R.ny = R.nz = 0.0f;
  R.pivot_ratio = R.c0 = 0.0;
  if (!framed) return R;
  R.kind = kMlsPlane;
  double hx = F.d0x, hy = F.d0y, hz = F.d0z, nx = F.nx, ny = F.ny, nz = F.nz;
  if (poly) {
    double c[kMlsBasis];
    if (mls_solve(a, c, R.pivot_ratio)) {
      R.c0 = c[0];
      if (!(fabs(c[0]) > (double)radius)) {
        R.kind = kMlsPoly;
        hx += c[0] * F.nx; hy += c[0] * F.ny; hz += c[0] * F.nz;
        const double su = c[1] * F.inv_r, sv = c[2] * F.inv_r;
        nx = F.nx - su * F.ux - sv * F.vx;
        ny = F.ny - su * F.uy - sv * F.vy;
        nz = F.nz - su * F.uz - sv * F.vz;
        const double len = sqrt(nx * nx + ny * ny + nz * nz);
        nx /= len; ny /= len; nz /= len;
      }
    }
  }
  face_viewpoint(nx, ny, nz, vx, vy, vz, qx, qy, qz);
  R.px = (float)((double)qx + hx);
  R.py = (float)((double)qy + hy);
  R.pz = (float)((double)qz + hz);
  R.nx = (float)nx; R.ny = (float)ny; R.nz = (float)nz;
  return R;
}

}  // namespace pcgx
