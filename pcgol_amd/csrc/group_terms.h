// group_terms.h -- the decisions of per-group geometry, shared by the device kernels (group_stats.hip) and the host test
// (tests/cpp/group_terms_host.cpp over the shim tests/cpp/host_shim): one expression, compiled by both.
// NOT in the reference: no parity, checked against the NumPy oracle's restatement (tests/group_oracle.py).
//
// Contract (include/pcgx.h, "group geometry"): the live-member test, the order-preserving keys of the min / max
// combines, the finish of a group's pivot-centred float64 sums into centroid and covariance, the eigen-solve (cov3.h's
// cyclic Jacobi at unit trace) with the order and the signs of the axes, and the oriented box from the extents.
// Every index is a compile-time constant: A and V stay in registers.
#pragma once
#include "cov3.h"

namespace pcgx {

// ------------------------------------------------------------------ live members
__device__ __forceinline__ bool group_finite(const float v) {
  uint32_t b;
  __builtin_memcpy(&b, &v, 4);
  return (b & 0x7f800000u) != 0x7f800000u;
}
// Is slot `id` of a tree of n points with these stored coordinates a live member?
__device__ __forceinline__ bool group_id_ok(const int64_t id, const int64_t n) { return id >= 0 && id < n; }
__device__ __forceinline__ bool group_point_ok(const float x, const float y, const float z) {
  return group_finite(x) && group_finite(y) && group_finite(z);
}

// ------------------------------------------------------------------ order-preserving keys
// a < b  =>  key(a) < key(b) as unsigned integers (-0 sorts below +0, which `<` calls equal); unkey(key(v)) has v's bits.
// An unsigned atomicMin / atomicMax over keys is a float min / max that does not depend on the order of the combines.
__device__ __forceinline__ uint32_t group_key_f32(const float v) {
  uint32_t b;
  __builtin_memcpy(&b, &v, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float group_unkey_f32(const uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float v;
  __builtin_memcpy(&v, &b, 4);
  return v;
}
__device__ __forceinline__ uint64_t group_key_f64(const double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double group_unkey_f64(const uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  __builtin_memcpy(&v, &b, 8);
  return v;
}
// the keys a min / a max starts from: above / below every value's key
constexpr uint32_t kGroupKeyMin32 = 0xffffffffu, kGroupKeyMax32 = 0u;
constexpr uint64_t kGroupKeyMin64 = 0xffffffffffffffffull, kGroupKeyMax64 = 0ull;

// ------------------------------------------------------------------ moments
// The pivot the sums of a group are centred on: the centre of its box, widened to double.
__device__ __forceinline__ double group_pivot(const float lo, const float hi) { return ((double)lo + (double)hi) * 0.5; }

// The pivot-centred sums of a group (or of a run of it): s = sum d (x, y, z), q = sum d d^T (xx, xy, xz, yy, yz, zz).
struct GroupSums {
  double sx, sy, sz, sxx, sxy, sxz, syy, syz, szz;
  int64_t n;
  __device__ __forceinline__ void clear() {
    sx = sy = sz = sxx = sxy = sxz = syy = syz = szz = 0.0;
    n = 0;
  }
  // one member at d = p - pivot (one rounding per sum: the products are fused into the additions)
  __device__ __forceinline__ void add(const double dx, const double dy, const double dz) {
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
  }
  __device__ __forceinline__ void merge(const GroupSums &o) {
    sx += o.sx; sy += o.sy; sz += o.sz;
    sxx += o.sxx; sxy += o.sxy; sxz += o.sxz; syy += o.syy; syz += o.syz; szz += o.szz;
    n += o.n;
  }
};

// centroid = pivot + s / n; cov = q / n - m m^T (xx, xy, xz, yy, yz, zz), m = s / n; a.n >= 1
__device__ __forceinline__ void group_finish(const GroupSums &a, const double px, const double py, const double pz,
                                             double (&centroid)[3], double (&cov)[6]) {
  const double n = (double)a.n;
  const double mx = a.sx / n, my = a.sy / n, mz = a.sz / n;
  centroid[0] = px + mx;
  centroid[1] = py + my;
  centroid[2] = pz + mz;
  cov[0] = a.sxx / n - mx * mx;
  cov[1] = a.sxy / n - mx * my;
  cov[2] = a.sxz / n - mx * mz;
  cov[3] = a.syy / n - my * my;
  cov[4] = a.syz / n - my * mz;
  cov[5] = a.szz / n - mz * mz;
}

// ------------------------------------------------------------------ the principal frame
// Turns a unit vector so that its component of largest magnitude is positive; on a tie the first such component decides.
__device__ __forceinline__ void group_sign(double &x, double &y, double &z) {
  const double ax = fabs(x), ay = fabs(y), az = fabs(z);
  const double lead = (ax >= ay && ax >= az) ? x : (ay >= az ? y : z);
  if (lead < 0.0) {
    x = -x;
    y = -y;
    z = -z;
  }
}

// eig[3]: the eigenvalues of cov, descending (equal ones in the order of their diagonal position); axes[9]: the unit
// eigenvectors as rows in that order, axes 0 and 1 signed by group_sign, axis 2 = axis 0 x axis 1.  A trace that is
// not positive and finite (every member at one place; an overflow): eig = 0, axes = identity.
__device__ __forceinline__ void group_frame(const double (&cov)[6], double (&eig)[3], double (&axes)[9]) {
  const double tr = cov[0] + cov[3] + cov[5];
  if (!(tr > 0.0) || !(tr < (double)__builtin_inff())) {
    eig[0] = eig[1] = eig[2] = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) axes[k] = (k % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  // cov3.h's solve (norm_acc_solve), all three pairs kept: unit trace, cyclic sweeps until nothing is left to rotate
  const double sc = 1.0 / tr;
  double A[3][3], V[3][3];
  A[0][0] = cov[0] * sc; A[0][1] = cov[1] * sc; A[0][2] = cov[2] * sc;
  A[1][1] = cov[3] * sc; A[1][2] = cov[4] * sc; A[2][2] = cov[5] * sc;
  A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
    if (fabs(A[0][1]) < 1e-18) A[0][1] = A[1][0] = 0.0;
    if (fabs(A[0][2]) < 1e-18) A[0][2] = A[2][0] = 0.0;
    if (fabs(A[1][2]) < 1e-18) A[1][2] = A[2][1] = 0.0;
    if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
    jacobi_rotate<0, 1>(A, V);
    jacobi_rotate<0, 2>(A, V);
    jacobi_rotate<1, 2>(A, V);
  }
  const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
  // the largest (the first of equal ones), the smallest (the last of equal ones), and the one left
  const int hi = (e0 >= e1 && e0 >= e2) ? 0 : (e1 >= e2 ? 1 : 2);
  const int lo = (e2 <= e0 && e2 <= e1) ? 2 : (e1 <= e0 ? 1 : 0);
  const int mid = 3 - hi - lo;
#define PCGX_GROUP_PICK(k, a, b, c) ((k) == 0 ? (a) : ((k) == 1 ? (b) : (c)))
  eig[0] = PCGX_GROUP_PICK(hi, e0, e1, e2) * tr;
  eig[1] = PCGX_GROUP_PICK(mid, e0, e1, e2) * tr;
  eig[2] = PCGX_GROUP_PICK(lo, e0, e1, e2) * tr;
  double ax = PCGX_GROUP_PICK(hi, V[0][0], V[0][1], V[0][2]), ay = PCGX_GROUP_PICK(hi, V[1][0], V[1][1], V[1][2]),
         az = PCGX_GROUP_PICK(hi, V[2][0], V[2][1], V[2][2]);
  double bx = PCGX_GROUP_PICK(mid, V[0][0], V[0][1], V[0][2]), by = PCGX_GROUP_PICK(mid, V[1][0], V[1][1], V[1][2]),
         bz = PCGX_GROUP_PICK(mid, V[2][0], V[2][1], V[2][2]);
#undef PCGX_GROUP_PICK
  const double la = sqrt(ax * ax + ay * ay + az * az), lb = sqrt(bx * bx + by * by + bz * bz);
  ax /= la; ay /= la; az /= la;
  bx /= lb; by /= lb; bz /= lb;
  group_sign(ax, ay, az);
  group_sign(bx, by, bz);
  axes[0] = ax; axes[1] = ay; axes[2] = az;
  axes[3] = bx; axes[4] = by; axes[5] = bz;
  axes[6] = ay * bz - az * by;
  axes[7] = az * bx - ax * bz;
  axes[8] = ax * by - ay * bx;
}

// ------------------------------------------------------------------ the oriented box
// One member's extent along one axis: (p - centroid) . axis in float64
__device__ __forceinline__ double group_extent(const float px, const float py, const float pz, const double (&c)[3],
                                               const double ax, const double ay, const double az) {
  return (((double)px - c[0]) * ax + ((double)py - c[1]) * ay) + ((double)pz - c[2]) * az;
}
// lo[k], hi[k]: the least and the greatest extent along axis k -> centre xyz, then the half-extents
__device__ __forceinline__ void group_obb(const double (&c)[3], const double (&axes)[9], const double (&lo)[3],
                                          const double (&hi)[3], double (&obb)[6]) {
  const double m0 = (hi[0] + lo[0]) * 0.5, m1 = (hi[1] + lo[1]) * 0.5, m2 = (hi[2] + lo[2]) * 0.5;
  obb[0] = c[0] + ((m0 * axes[0] + m1 * axes[3]) + m2 * axes[6]);
  obb[1] = c[1] + ((m0 * axes[1] + m1 * axes[4]) + m2 * axes[7]);
  obb[2] = c[2] + ((m0 * axes[2] + m1 * axes[5]) + m2 * axes[8]);
  obb[3] = (hi[0] - lo[0]) * 0.5;
  obb[4] = (hi[1] - lo[1]) * 0.5;
  obb[5] = (hi[2] - lo[2]) * 0.5;
}

}  // namespace pcgx
