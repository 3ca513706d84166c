// fpfh_match_terms.h -- the distance between two FPFH rows and which rows take part in matching, shared by the device
// kernels (fpfh_match.hip) and the host test (tests/cpp/match_terms_host.cpp): one expression, compiled by both.  NOT in
// the reference: no parity, checked against the NumPy oracle's restatement (tests/match_oracle.py).
//
// Contract (include/pcgx.h, "FPFH matching"): float32, left to right, nothing fused (build with -ffp-contract=off, the
// rule of ref_dist_sq):
//   acc = 0;  for k = 0 .. 32:  d = a[k] - b[k];  acc = acc + d * d;     D(a, b) = acc
// a[k] - b[k] and b[k] - a[k] differ in sign only, so D(a, b) and D(b, a) have the same bits.  A row is usable when all
// 33 values are finite and at least one is not zero (-0.0 is zero).
#pragma once
#include "pcgx_math.h"

namespace pcgx {

constexpr int kMatchLen = 33;  // floats per row: what pcgx_kdtree_fpfh writes (fpfh_terms.h, kFpfhLen)

PCGX_HD float fpfh_row_dist_sq(const float *a, const float *b) {
  float acc = 0.0f;
  for (int k = 0; k < kMatchLen; k++) {
    const float d = a[k] - b[k];
    acc = acc + d * d;
  }
  return acc;
}

PCGX_HD bool fpfh_row_usable(const float *a) {
  const float inf = __builtin_inff();
  bool finite = true, any = false;
  for (int k = 0; k < kMatchLen; k++) {
    finite = finite && fabsf(a[k]) < inf;  // (false for NaN)
    any = any || a[k] != 0.0f;
  }
  return finite && any;
}

}  // namespace pcgx
