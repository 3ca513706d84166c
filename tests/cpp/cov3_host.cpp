// csrc/cov3.h on the host (tests/test_cov3_host.py): the moments as the kernels take them (NormAcc::add in list order,
// norm_acc_cov) and the unit-trace Jacobi solve (norm_acc_solve), over batches, through extern "C".
#include <stdint.h>

#include "cov3.h"

using namespace pcgx;

extern "C" {

// m lists back to back: list i is points[offs[i] .. offs[i + 1]) (xyz float32) about q[3 i ..] -> c6[6 i ..] (xx, xy,
// xz, yy, yz, zz) and tr[i] = xx + yy + zz, as covariance_finish / normals_finish form them
void cov3_moments(const float *points, const int64_t *offs, const float *q, int64_t m, double *c6, double *tr) {
  for (int64_t i = 0; i < m; i++) {
    NormAcc a;
    a.clear();
    for (int64_t j = offs[i]; j < offs[i + 1]; j++)
      a.add(points[3 * j], points[3 * j + 1], points[3 * j + 2], q[3 * i], q[3 * i + 1], q[3 * i + 2]);
    double A[3][3];
    norm_acc_cov(a, A);
    double *c = c6 + 6 * i;
    c[0] = A[0][0]; c[1] = A[0][1]; c[2] = A[0][2]; c[3] = A[1][1]; c[4] = A[1][2]; c[5] = A[2][2];
    tr[i] = A[0][0] + A[1][1] + A[2][2];
  }
}

// m matrices c6 with trace tr > 0 -> l0[i] (the returned smallest scaled eigenvalue), e[3 i ..] (the scaled diagonal)
// and u[3 i ..] (the unit eigenvector)
void cov3_solve(const double *c6, const double *tr, int64_t m, double *l0, double *e, double *u) {
  for (int64_t i = 0; i < m; i++) {
    const double *c = c6 + 6 * i;
    double A[3][3], V[3][3];
    A[0][0] = c[0]; A[0][1] = c[1]; A[0][2] = c[2]; A[1][1] = c[3]; A[1][2] = c[4]; A[2][2] = c[5];
    l0[i] = norm_acc_solve(A, V, tr[i], e[3 * i], e[3 * i + 1], e[3 * i + 2], u[3 * i], u[3 * i + 1], u[3 * i + 2]);
  }
}

}  // extern "C"
