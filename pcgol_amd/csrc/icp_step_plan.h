// What one ICP iteration launches, decided in one place: plan_step() maps the facts of a session at the start of a step
// (StepFacts) and the process's knobs (StepKnobs) to the step's launches as data (StepPlan).  Plain C++ on host values:
// no HIP, no session or tree type, no environment -- icp.hip gathers the facts and reads the knobs (step_knobs), and
// enqueues what the plan says (enqueue_corr, enqueue_sums); tests/test_icp_step_plan.py compiles this header with g++
// and compares the plan over the whole input space.
#pragma once
#include <cstdint>

namespace pcgx {

struct StepFacts {
  bool patched = false;           // the base has deletions: the reference's patched explicit tree is walked
  bool plane = false;             // point-to-plane session
  int32_t strict = 0;             // the reference's sequential float32 sums: 1 = strict.hip, 2 = the one-wave chain
  bool min_dist = false;          // MinDistSq > 0
  bool has_targets = false;       // nt > 0
  bool grid_enabled = false;      // the tree has a voxel grid and the grid is not switched off
  bool has_cert = false;          // ... with certificates (GridView::cert)
  bool have_match_caller = false; // d_orig_of / d_match_caller could be allocated (asked for by strict 1 steps only)
  bool caller_had_pairs = false;  // the step before this one left every pair in the caller's order too
  bool exchange = false;          // StrictWork::exchange: the summary kernel forms and exchanges the tile sums itself
  bool spec_walk = true;          // no speculated step of this session has met a target the grid could not answer
  int32_t host_iter = 0;          // Evaluates enqueued since the device's loop state was last written
  bool may_speculate = false;     // the caller looks at the step's outcome later (settle()): session_step only
  int32_t grid = 1;               // the session's launch grid of the walk (icp_grid)
};

struct StepKnobs {
  // Walk knobs of the ICP kernel (the hinted walk of iterations >= 1 profits from resolving wrong leaf predictions in
  // lockstep during the chunk preparation; the cold C2 walk does not)
  int32_t tight = 32;  // PCGX_ICP_TIGHT, 0..32 (32: the whole descent)
  int32_t chunks = 2;  // PCGX_ICP_CHUNKS, 1..64 chunks per refill section
  // Strict sessions behind a grid pass: the correspondence kernel is there for the few targets the grid could not
  // certify (none at C4) and forms no sums -- 128 workgroups instead of two per CU: the launch of 512 of them, 66 KB
  // of LDS each, cost 4-6 us per iteration to find nothing to do.
  int32_t left_blocks = 128;  // PCGX_ICP_LEFTOVER_BLOCKS, 8..4096, rounded down to a multiple of 8
  bool cert_on = true;        // PCGX_ICP_CERT (0: every pair is searched for, as before round 5)
  bool spec_on = true;        // PCGX_ICP_SPEC_WALK (0: the leftover walk behind every grid pass)
  int32_t fused_from = 2;     // PCGX_ICP_FUSED_FROM, 0..2^30 (0: never): see StepPlan::certify
  // test aids, handed to the kernels as they are (0: off)
  int32_t test_force_walk = 0;        // PCGX_TEST_ICP_FORCE_WALK: icp_grid_kernel
  int32_t test_fused_search = 0;      // PCGX_TEST_ICP_FUSED_SEARCH: CertifiedTerms::test_force_walk
  int32_t test_fused_grid_walk = 0;   // PCGX_TEST_ICP_FUSED_GRID_WALK: CertifiedTerms::test_force_grid_walk
};

enum CorrForm : int32_t {
  kCorrPatched = 0,   // icp_corr_xkernel on the patched explicit tree, nothing else
  kCorrWalk = 1,      // icp_corr_kernel walks the tree for every target
  kCorrGridWalk = 2,  // icp_grid_kernel, then icp_corr_kernel for the targets the grid left over
  kCorrGrid = 3,      // icp_grid_kernel only (no_walk)
  kCorrNone = 4,      // nothing in front of the summary kernel: it certifies or searches the pairs itself (certify)
};

struct StepPlan {
  CorrForm corr = kCorrWalk;
  int32_t n_corr = 1;           // workgroups of icp_corr_kernel, and the walk-list segments icp_grid_kernel fills
  bool write_caller = false;    // the correspondence kernels leave every pair in the caller's target order as well
  bool tile_sums = false;       // ... and their workgroups form the strict sums' float64 tile sums on their way out
  bool grid_has_caller_pairs = false;  // icp_grid_kernel<false, false, false>: d_match_caller holds the last step's pairs
  bool cert = false;            // certificates are written and tested (d_match_cert)
  bool no_walk = false;         // a speculated step: no leftover walk (the session notes spec_pending / spec_stream)
  bool certify = false;         // ... and no grid pass either: CertifiedTerms go to strict_enqueue
  bool sums_caller = false;     // the strict sums read {match_caller, none} (else {match, pos_of}: a gather)
  bool have_tile_sums = false;  // strict_enqueue finds the tile sums formed
  bool first_iter = false;      // the Fit's first Evaluate (strict 1: the repair pass)
  bool next_caller_had_pairs = false;  // the next step's StepFacts::caller_had_pairs
};

inline StepPlan plan_step(const StepFacts &f, const StepKnobs &k) {
  StepPlan p;
  p.n_corr = f.grid;
  p.first_iter = f.host_iter == 0;
  if (f.patched) {  // (without hints from earlier iterations, and without the caller's order: the sums gather)
    p.corr = kCorrPatched;
    return p;
  }
  // the strict sums run in the caller's target order: the kernels below also leave every pair there
  const bool caller = f.strict == 1 && !f.plane && f.has_targets && f.have_match_caller;
  p.write_caller = p.sums_caller = p.next_caller_had_pairs = caller;
  const bool grid = f.grid_enabled && !f.min_dist && f.has_targets;
  // with the grid pass before it the correspondence kernel finds (nearly) every pair in place: its workgroups
  // form the strict sums' tile sums on their way out (else strict_tilesum_kernel does, after this launch)
  // (unless the summary kernel forms and exchanges them itself, StrictWork::exchange: the default)
  p.tile_sums = p.have_tile_sums = grid && caller && !f.exchange;
  if (grid && f.strict && !f.plane && f.grid > k.left_blocks) p.n_corr = k.left_blocks;  // (StepKnobs::left_blocks)
  p.cert = grid && k.cert_on && f.has_cert;
  p.grid_has_caller_pairs = grid && f.strict && !f.plane && f.caller_had_pairs;
  // The leftover walk behind the grid pass finds nothing to do in iteration after iteration (C4: never anything), and
  // its launch is 5 us of a 70 us step.  From a Fit's second Evaluate on it is therefore NOT launched behind a strict
  // session's grid pass -- on the speculation that the grid answers every target; a target it cannot answer ends the
  // step on the device (icp_grid_kernel: `done` 2) and settle() enqueues it again with the walk, as every step after it.
  p.no_walk = f.may_speculate && k.spec_on && f.spec_walk && grid && f.strict == 1 && !f.plane && f.host_iter >= 1 &&
              !p.tile_sums;
  // From a Fit's K-th Evaluate on (PCGX_ICP_FUSED_FROM, 0: never) not even the grid pass runs: 98.5 % of the targets
  // keep their partner from the third iteration on, and the summary kernel reads every target and its partner anyway --
  // it tests the certificates and searches the rest itself (strict.hip, strict_sum_kernel<., ., true>).  The same
  // speculation as no_walk: a target the grid cannot answer ends the step with `done` 2, settle() enqueues it again.
  // (K = 2: 0.0673 ms a C4 step against 0.0680 with K = 3, where iteration 2 still runs the grid pass: DESIGN 3.1)
  p.certify = p.no_walk && k.fused_from > 0 && f.host_iter >= k.fused_from && p.cert && f.caller_had_pairs && caller &&
              f.exchange;
  p.corr = p.certify ? kCorrNone : p.no_walk ? kCorrGrid : grid ? kCorrGridWalk : kCorrWalk;
  return p;
}

}  // namespace pcgx
