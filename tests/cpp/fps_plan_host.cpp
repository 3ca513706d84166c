// csrc/fps_plan.h on the host (tests/test_fps_plan.py): plan_fps over arrays of cases.  The header needs no shim: it
// includes neither HIP nor anything of the library.
#include "fps_plan.h"

using namespace pcgx;

// out: [kOut][n] int64: picks, tile, tiles, wg_tiles, workgroups, then the bytes of every buffer in FpsBuf's order
enum { kOut = 5 + kFpsBufs };

extern "C" int32_t fps_plan_rows(int32_t out[2]) {
  out[0] = kOut;
  out[1] = kFpsBufs;
  return 0;
}

extern "C" void fps_plan_facts(int64_t out[4]) {
  const FpsFacts f;
  out[0] = f.tile;
  out[1] = f.waves;
  out[2] = f.max_workgroups;
  out[3] = f.wave;
}

extern "C" void fps_plan_cases(const int64_t *len, const int64_t *count, int64_t n, int64_t *out) {
  for (int64_t i = 0; i < n; i++) {
    const FpsPlan p = plan_fps(len[i], count[i]);
    out[0 * n + i] = p.picks;
    out[1 * n + i] = p.tile;
    out[2 * n + i] = p.tiles;
    out[3 * n + i] = p.wg_tiles;
    out[4 * n + i] = p.workgroups;
    for (int b = 0; b < kFpsBufs; b++) out[(5 + b) * n + i] = (int64_t)p.bytes[b];
  }
}
