// csrc/pose_score_plan.h on the host (tests/test_score_plan.py): plan_score over arrays of cases.  The header needs no
// shim: it includes neither HIP nor anything of the library.
#include "pose_score_plan.h"

using namespace pcgx;

// in: [kIn][n] int64, one row per input in the order below; out: [kOut][n] int64: path, tiles, chunk, nchunks, order,
// then the bytes of every buffer in ScoreBuf's order
enum { kIn = 9, kOut = 5 + kScoreBufs };

extern "C" int32_t score_plan_rows(int32_t out[3]) {
  out[0] = kIn;
  out[1] = kOut;
  out[2] = kScoreBufs;
  return 0;
}

extern "C" void score_plan_facts(int64_t out[5]) {
  const ScoreFacts f;
  out[0] = f.tile;
  out[1] = f.wave;
  out[2] = f.pair_budget;
  out[3] = f.max_chunk;
  out[4] = (int64_t)f.partial_rec;
}

extern "C" void score_plan_cases(const int64_t *in, int64_t n, int64_t *out) {
  for (int64_t i = 0; i < n; i++) {
    const auto at = [&](int row) { return in[row * n + i]; };
    ScoreInputs s;
    s.n = at(0);
    s.K = at(1);
    s.grid = at(2) != 0;
    s.deletions = at(3) != 0;
    s.empty = at(4) != 0;
    s.forced_chunk = at(5);
    s.sort_workspace = (size_t)at(6);
    s.have_counts = at(7) != 0;
    s.have_sums = at(8) != 0;
    const ScorePlan p = plan_score(s);
    out[0 * n + i] = p.path;
    out[1 * n + i] = p.tiles;
    out[2 * n + i] = p.chunk;
    out[3 * n + i] = p.nchunks;
    out[4 * n + i] = p.order ? 1 : 0;
    for (int b = 0; b < kScoreBufs; b++) out[(5 + b) * n + i] = (int64_t)p.bytes[b];
  }
}
