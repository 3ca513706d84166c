// keypoint_terms.h -- the two decisions of keypoint detection, shared by the device kernels (normals.hip: saliency;
// keypoints.hip: suppression) and the host test (tests/cpp/keypoint_terms_host.cpp): one expression, compiled by both.
// NOT in the reference: no parity, checked against the NumPy oracle's restatement (tests/keypoints_oracle.py).
//
// Contract (include/pcgx.h, "keypoints"): float32, every product rounded once, nothing fused (build with
// -ffp-contract=off, the rule of ref_dist_sq).
#pragma once
#include "pcgx_math.h"

namespace pcgx {

// ISS saliency of a point whose covariance has the float32 eigenvalues l0 <= l1 <= l2: l0 where the point is salient
// (l0 > 0, l1 < gamma_21 * l2, l0 < gamma_32 * l1, both products float32), else 0.  A NaN anywhere: 0.
PCGX_HD float iss_saliency(const float l0, const float l1, const float l2, const float gamma_21, const float gamma_32) {
  const float t21 = gamma_21 * l2;
  const float t32 = gamma_32 * l1;
  return (l0 > 0.0f && l1 < t21 && l0 < t32) ? l0 : 0.0f;
}

// May a point of score s be a local maximum at all?  NaN, 0 (either sign) and negative scores never; +inf may.
PCGX_HD bool keypoint_candidate(const float s) { return s > 0.0f; }

// Does neighbour j (score sj) beat point i (score si)?  A larger score does; an equal one with the smaller id does
// (ties go to the smaller id, as in pcgx_kdtree_knearest).  A NaN on either side beats nobody; j == i beats nobody.
PCGX_HD bool keypoint_beats(const float sj, const int64_t j, const float si, const int64_t i) {
  return sj > si || (sj == si && j < i);
}

}  // namespace pcgx
