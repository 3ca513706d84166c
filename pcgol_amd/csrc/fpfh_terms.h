// fpfh_terms.h -- one pair's bins of the FPFH extension (Rusu, Blodow, Beetz 2009), shared by the device kernel
// (fpfh.hip, spfh_kernel) and the host test (tests/cpp/fpfh_terms_host.cpp): one expression, compiled by both.  NOT in
// the reference: no parity, checked against the NumPy oracle's restatement (tests/fpfh_oracle.py).
//
// Contract (include/pcgx.h, "FPFH descriptors"): query s (point ps, normal ns), neighbour t (pt, nt), in float64 from
// the float32 inputs widened:
//   d = pt - ps, f4 = |d|, a1 = ns . d / f4, a2 = nt . d / f4;
//   |a1| < |a2|: (n1, n2, d, f3) = (nt, ns, -d, -a2), else (ns, nt, d, a1)   (the source is the point whose normal
//   makes the smaller angle with the line between the two; comparing magnitudes is the same decision as comparing
//   acos);
//   v = d x n1, v /= |v|, w = n1 x v, f2 = v . n2, f1 = atan2(w . n2, n1 . n2);
//   b1 = clamp(floor(11 (f1 + pi) / 2 pi), 0, 10), b2 = clamp(floor(11 (f2 + 1) / 2), 0, 10), b3 likewise from f3.
// The pair is invalid (false is returned, nothing is written) when the float32 DistSq is 0 (the point itself, exact
// duplicates), when a normal is zero or not finite, or when |v| == 0 (d parallel to n1).  Normals are used as given.
//
// No product feeds a sum the bins' decisions hang on except through a handful of float64 roundings, so whether the
// compiler contracts a * b + c into fma moves a bin only where the scaled value is within ~1e-15 of an integer: the
// tests' admissible sets (within 1e-9) cover either choice.
#pragma once
#include "pcgx_math.h"

namespace pcgx {

constexpr int kFpfhBins = 11;            // per feature
constexpr int kFpfhLen = 3 * kFpfhBins;  // f1's bins, then f2's, then f3's

// clamp(floor(x), 0, 10); NaN -> 0 (cannot happen for a valid pair: every input is finite)
PCGX_HD int fpfh_bin(const double x) {
  if (!(x >= 0.0)) return 0;
  if (x >= (double)(kFpfhBins - 1)) return kFpfhBins - 1;
  return (int)x;
}

// finite and not (0, 0, 0)
PCGX_HD bool fpfh_normal_ok(const float x, const float y, const float z) {
  const float inf = __builtin_inff();
  if (!(fabsf(x) < inf) || !(fabsf(y) < inf) || !(fabsf(z) < inf)) return false;
  return x != 0.0f || y != 0.0f || z != 0.0f;
}

PCGX_HD bool fpfh_terms(const float psx, const float psy, const float psz, const float nsx, const float nsy,
                        const float nsz, const float ptx, const float pty, const float ptz, const float ntx,
                        const float nty, const float ntz, int &b1, int &b2, int &b3) {
  {  // the reference's float32 DistSq (mat/vec3.go), as range_enum.h's ref_dist_sq
    const float ex = ptx - psx, ey = pty - psy, ez = ptz - psz;
    const float s = ex * ex + ey * ey;
    if (s + ez * ez == 0.0f) return false;
  }
  if (!fpfh_normal_ok(nsx, nsy, nsz) || !fpfh_normal_ok(ntx, nty, ntz)) return false;
  double dx = (double)ptx - (double)psx, dy = (double)pty - (double)psy, dz = (double)ptz - (double)psz;
  const double f4 = sqrt((dx * dx + dy * dy) + dz * dz);
  if (!(f4 > 0.0)) return false;  // (DistSq > 0 in float32: d != 0, and |d|^2 >= 2^-298 does not underflow in float64)
  const double a1 = (((double)nsx * dx + (double)nsy * dy) + (double)nsz * dz) / f4;
  const double a2 = (((double)ntx * dx + (double)nty * dy) + (double)ntz * dz) / f4;
  double n1x, n1y, n1z, n2x, n2y, n2z, f3;
  if (fabs(a1) < fabs(a2)) {
    n1x = ntx; n1y = nty; n1z = ntz;
    n2x = nsx; n2y = nsy; n2z = nsz;
    dx = -dx; dy = -dy; dz = -dz;
    f3 = -a2;
  } else {
    n1x = nsx; n1y = nsy; n1z = nsz;
    n2x = ntx; n2y = nty; n2z = ntz;
    f3 = a1;
  }
  double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
  const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
  if (!(vn > 0.0)) return false;
  vx /= vn; vy /= vn; vz /= vn;
  const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
  const double f2 = (vx * n2x + vy * n2y) + vz * n2z;
  const double f1 = atan2((wx * n2x + wy * n2y) + wz * n2z, (n1x * n2x + n1y * n2y) + n1z * n2z);
  const double pi = 3.14159265358979323846;
  b1 = fpfh_bin((double)kFpfhBins * (f1 + pi) / (2.0 * pi));
  b2 = fpfh_bin((double)kFpfhBins * (f2 + 1.0) / 2.0);
  b3 = fpfh_bin((double)kFpfhBins * (f3 + 1.0) / 2.0);
  return true;
}

}  // namespace pcgx
