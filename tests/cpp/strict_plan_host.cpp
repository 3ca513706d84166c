// csrc/strict_plan.h on the host (tests/test_strict_plan.py): the three plans over arrays of cases.  The header needs no
// shim: it includes neither HIP nor anything of the library.
#include "strict_plan.h"

using namespace pcgx;

enum { kLayoutIn = 2, kLayoutOut = 5 + 2 * kStrictRegions + 10, kLaunchIn = 18, kLaunchOut = 11, kShardIn = 5, kShardOut = 4 };

extern "C" int32_t strict_plan_rows(int32_t out[6]) {
  const int32_t rows[6] = {kLayoutIn, kLayoutOut, kLaunchIn, kLaunchOut, kShardIn, kShardOut};
  for (int i = 0; i < 6; i++) out[i] = rows[i];
  return kStrictRegions;
}

// the facts the plans default to, in the order of StrictFacts
extern "C" void strict_plan_facts(int64_t out[12]) {
  const StrictFacts f;
  const int64_t v[12] = {f.rows, f.tile, f.lanes, f.chain_tiles, f.aux_shards, f.cand, f.repair_block, f.repair_min_tiles,
                         f.job_roles, (int64_t)f.tile_rec, (int64_t)f.leaf_aux, (int64_t)f.job_desc};
  for (int i = 0; i < 12; i++) out[i] = v[i];
}

// in: [2][n] nt, slots_per_shard; out: [kLayoutOut][n] ntiles, ntiles_pad, nchunks, naux, total, the regions' offsets,
// their sizes, zero_create as (first, last) x 3, zero_reset as (first, last) x 2
extern "C" void strict_layout_cases(const int64_t *in, int64_t n, int64_t *out) {
  for (int64_t i = 0; i < n; i++) {
    StrictKnobs k;
    k.slots_per_shard = (int32_t)in[1 * n + i];
    const StrictLayout L = plan_strict_layout(in[0 * n + i], k);
    int row = 0;
    const auto put = [&](int64_t v) { out[row++ * n + i] = v; };
    put(L.ntiles), put(L.ntiles_pad), put(L.nchunks), put(L.naux), put((int64_t)L.total);
    for (int r = 0; r < kStrictRegions; r++) put((int64_t)L.region[r].offset);
    for (int r = 0; r < kStrictRegions; r++) put((int64_t)L.region[r].bytes);
    for (const StrictLayout::Run &z : L.zero_create) put(z.first), put(z.last);
    for (const StrictLayout::Run &z : L.zero_reset) put(z.first), put(z.last);
  }
}

// in: [18][n] form, exchange, have_tile_sums, first_iter, certify, pos_of present, naux, ntiles, nchunks, nrows, rank, world,
// spec_depth, selfcheck, spec_on, repair_on, local_failed, fuse_update; out: [11][n] the fields of StrictLaunches in their order
extern "C" void strict_launch_cases(const int64_t *in, int64_t n, int64_t *out) {
  for (int64_t i = 0; i < n; i++) {
    const auto at = [&](int row) { return in[row * n + i]; };
    StrictKnobs k;
    StrictStep s;
    k.exchange = (int32_t)at(1);
    s.have_tile_sums = at(2) != 0;
    s.first_iter = at(3) != 0;
    s.certify = at(4) != 0;
    s.caller_order = at(5) == 0;
    s.naux = (int32_t)at(6);
    s.ntiles = at(7);
    s.nchunks = (int32_t)at(8);
    s.nrows = (int32_t)at(9);
    s.rank = (int32_t)at(10);
    s.world = (int32_t)at(11);
    k.spec_depth = (int32_t)at(12);
    k.selfcheck = (int32_t)at(13);
    k.spec_on = at(14) != 0;
    k.repair_on = at(15) != 0;
    s.local_failed = at(16) != 0;
    s.fuse_update = at(17) != 0;
    const StrictLaunches L = plan_strict_launches((StrictForm)at(0), s, k);
    const int64_t v[kLaunchOut] = {L.live, L.tilesum, L.summary, L.exchange, L.bases_behind_summary, L.ring_err_grid,
                                   L.repair_grid, L.jobs_grid, L.chain, L.chain_grid, L.fuse_update};
    for (int r = 0; r < kLaunchOut; r++) out[r * n + i] = v[r];
  }
}

// in: [5][n] have_block, block_world, block_ring, world, want_ring; out: [4][n] allocate, zero, bytes, ring
extern "C" void strict_shard_cases(const int64_t *in, int64_t n, int64_t *out) {
  for (int64_t i = 0; i < n; i++) {
    const ShardPlan p = plan_shard(in[i] != 0, (int)in[n + i], in[2 * n + i] != 0, (int)in[3 * n + i], in[4 * n + i] != 0);
    const int64_t v[kShardOut] = {p.allocate, p.zero, (int64_t)p.bytes, p.ring};
    for (int r = 0; r < kShardOut; r++) out[r * n + i] = v[r];
  }
}
