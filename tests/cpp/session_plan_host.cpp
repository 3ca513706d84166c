// csrc/icp_session_plan.h on the host (tests/test_icp_session_plan.py): plan_session over arrays of cases.  The header
// needs no shim: it includes neither HIP nor anything of the library.
#include "icp_session_plan.h"

using namespace pcgx;

// in: [kIn][n] int64, one row per fact in the order below; out: [kOut][n] int64: the plan's fields, then its sizes
enum { kIn = 15, kOut = 10 + kSessionBuffers };

extern "C" int32_t session_plan_rows(int32_t *in, int32_t *out) {
  *in = kIn;
  *out = kOut;
  return kSessionBuffers;
}

extern "C" void session_plan_cases(const int64_t *in, int64_t n, int64_t *out) {
  for (int64_t i = 0; i < n; i++) {
    const auto at = [&](int row) { return in[row * n + i]; };
    SessionFacts f;
    f.normals = at(0) != 0;
    f.covariances = at(1) != 0;
    f.sums_mode = (int32_t)at(2);
    f.strict_override = (int32_t)at(3);
    f.nt = at(4);
    f.n_base = at(5);
    f.patched = at(6) != 0;
    f.has_nan = at(7) != 0;
    f.small_on = at(8) != 0;
    f.small_eligible = at(9) != 0;
    f.small_wants_order = at(10) != 0;
    f.grid = (int32_t)at(11);
    f.num_cu = (int32_t)at(12);
    f.caller_sums = at(13) != 0;
    f.state_bytes = (size_t)at(14);
    const SessionPlan p = plan_session(f);
    const int64_t fields[10] = {p.gicp, p.plane, p.strict, p.strict_explicit, p.small, p.gicp_grid, p.n_sums,
                                p.start_values, p.nt_pad, p.small_buffers};
    for (int r = 0; r < 10; r++) out[r * n + i] = fields[r];
    for (int b = 0; b < kSessionBuffers; b++) out[(10 + b) * n + i] = (int64_t)p.bytes[b];
  }
}

extern "C" void session_block_sizes(int32_t out[2]) {
  out[0] = kIcpGridBlock;
  out[1] = kGicpBlock;
}
