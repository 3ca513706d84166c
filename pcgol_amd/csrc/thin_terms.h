// thin_terms.h -- the decisions of minimum-distance subsampling, shared by the device kernels (thin.hip) and the host
// test (tests/cpp/thin_terms_host.cpp): one expression, compiled by both.
// NOT in the reference: no parity, checked against the NumPy oracle's restatement (tests/thin_oracle.py).
//
// Contract (include/pcgx.h, "minimum-distance subsampling"): the kept set is the lexicographically first maximal
// independent set of the radius graph on the eligible points, under a total order that is either the partner rule's
// (hash(seed, id), id) (shape_terms.h) or the keypoints' "j beats i" on a score (keypoint_terms.h); a dropped point goes
// with the kept neighbour of the smallest (DistSq, id) (dbscan_terms.h).  Nothing here is new arithmetic: the three
// comparisons are forwarded, so their bits are the ones the existing host tests pin.
#pragma once
#include "dbscan_terms.h"
#include "keypoint_terms.h"
#include "shape_terms.h"

namespace pcgx {

// a point's state, one byte by id
enum ThinState : uint8_t { kThinUndecided = 0, kThinKept = 1, kThinDropped = 2, kThinIneligible = 3 };

// what owner[] holds besides a kept point's id
constexpr int32_t kThinNoOwner = -1;   // a point outside E
constexpr int32_t kThinNotRun = -2;    // the owner pass did not run: points were still undecided

// rounds a device call enqueues where the caller says 0, and the host form's batch
constexpr int32_t kThinDefaultRounds = 32;

// May the score s take part?  No score at all (hash mode) always may; a NaN never.
PCGX_HD bool thin_score_ok(const bool has_score, const float s) { return !has_score || s == s; }

// Is the point in E?  met_self: the enumeration of its own neighbourhood reported the point itself, which it does for
// a live point with three finite coordinates and for no other (a deleted id is in no tree; NaN and inf - inf compare
// below no bound).
PCGX_HD bool thin_eligible(const bool met_self, const bool has_score, const float s) {
  return met_self && thin_score_ok(has_score, s);
}

// Does j come before i in the priority order?  Hash mode: the smaller shape_partner_key(seed, .), whose low word is the
// id, so no two points tie.  Score mode: keypoint_beats, the larger score, equal ones (-0 == +0) by the smaller id; both
// scores are no NaN here (thin_score_ok).  j == i: false in both modes.
PCGX_HD bool thin_before(const bool has_score, const uint32_t seed, const float sj, const uint32_t j, const float si,
                         const uint32_t i) {
  if (has_score) return keypoint_beats(sj, (int64_t)j, si, (int64_t)i);
  return shape_partner_key(seed, j) < shape_partner_key(seed, i);
}

// One round's decision for an undecided point from the two bits accumulated over its neighbours that come before it:
// one of them is KEPT; one of them is UNDECIDED.  Both read from the states as the previous round left them.
PCGX_HD uint8_t thin_decide(const bool eligible, const bool kept_before, const bool undecided_before) {
  if (!eligible) return kThinIneligible;
  if (kept_before) return kThinDropped;
  return undecided_before ? kThinUndecided : kThinKept;
}

// Does the kept neighbour (d, id) beat the best owner so far?  dbscan_terms.h's rule for the nearest core point.
PCGX_HD bool thin_owner_beats(const float d, const uint32_t id, const float best_d, const uint32_t best_id) {
  return dbscan_beats(d, id, best_d, best_id);
}

}  // namespace pcgx
