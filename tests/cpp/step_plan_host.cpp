// csrc/icp_step_plan.h on the host (tests/test_icp_step_plan.py): plan_step over arrays of cases.  The header needs no
// shim: it includes neither HIP nor anything of the library.
#include "icp_step_plan.h"

using namespace pcgx;

// in: [kIn][n] int16, one row per fact or knob in the order below; out: [kOut][n] int16, one row per plan field
enum { kIn = 18, kOut = 12 };

extern "C" void step_plan_cases(const int16_t *in, int64_t n, int16_t *out) {
  for (int64_t i = 0; i < n; i++) {
    const auto at = [&](int row) { return in[row * n + i]; };
    StepFacts f;
    f.patched = at(0) != 0;
    f.plane = at(1) != 0;
    f.strict = at(2);
    f.min_dist = at(3) != 0;
    f.has_targets = at(4) != 0;
    f.grid_enabled = at(5) != 0;
    f.has_cert = at(6) != 0;
    f.have_match_caller = at(7) != 0;
    f.caller_had_pairs = at(8) != 0;
    f.exchange = at(9) != 0;
    f.spec_walk = at(10) != 0;
    f.host_iter = at(11);
    f.may_speculate = at(12) != 0;
    f.grid = at(13);
    StepKnobs k;
    k.cert_on = at(14) != 0;
    k.spec_on = at(15) != 0;
    k.fused_from = at(16);
    k.left_blocks = at(17);
    const StepPlan p = plan_step(f, k);
    const int16_t fields[kOut] = {(int16_t)p.corr, (int16_t)p.n_corr, p.write_caller, p.tile_sums, p.grid_has_caller_pairs,
                                  p.cert, p.no_walk, p.certify, p.sums_caller, p.have_tile_sums, p.first_iter,
                                  p.next_caller_had_pairs};
    for (int r = 0; r < kOut; r++) out[r * n + i] = fields[r];
  }
}

// the knobs nobody set: tight, chunks, left_blocks, cert_on, spec_on, fused_from, the three test aids
extern "C" void step_knob_defaults(int32_t out[9]) {
  const StepKnobs k;
  const int32_t v[9] = {k.tight, k.chunks, k.left_blocks, k.cert_on, k.spec_on, k.fused_from, k.test_force_walk,
                        k.test_fused_search, k.test_fused_grid_walk};
  for (int r = 0; r < 9; r++) out[r] = v[r];
}
