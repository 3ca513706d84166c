// What the host side of strict.hip allocates and launches, decided in one place: plan_strict_layout() carves a session's
// one block into named regions, plan_strict_launches() says which kernels a step runs, with which grid, in each of its
// three forms, plan_shard() what becomes of the block a sharded step exchanges through.  Plain C++ on host values: no
// HIP, no environment, no StrictBuffers -- strict.hip reads the environment (strict_knobs), allocates, and enqueues what
// the plans say; tests/test_strict_plan.py compiles this header with g++ and compares the plans over their input space.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pcgx {

// the kernels' constants and record sizes the plans depend on (strict_sum.h, strict_terms.h, strict.hip: they need
// HIP); strict.hip static_asserts every one against its definition
struct StrictFacts {
  int32_t rows = 9;                 // kStrictRows
  int32_t tile = 2048;              // kTile: terms per tile
  int32_t lanes = 64;               // kLanes: leaves per tile
  int32_t chain_tiles = 512;        // kChainTiles: tiles per chunk of the chain kernel
  int32_t aux_shards = 64;          // kAuxShards
  int32_t cand = 768;               // kCand
  int32_t repair_block = 512;       // kRepairBlock
  int64_t repair_min_tiles = 1024;  // kRepairMinTiles
  int32_t job_roles = 3;            // kJobRoles
  size_t tile_rec = 64, leaf_aux = 96, job_desc = 16;  // sizeof(TileRec), sizeof(LeafAux), sizeof(JobDesc)
};

// what PCGX_STRICT_* and PCGX_TEST_SPEC_MISS say (strict.hip, strict_knobs)
struct StrictKnobs {
  int32_t spec_depth = 4;  // _SPEC_DEPTH: a walker with this many walks in front of it walks ahead of its wait
  // _SELFCHECK 1, _TRACE 2, _NOSPEC 4, _CLOCKS 8, PCGX_TEST_SPEC_MISS 16
  // (4: the chain kernel ignores the candidate tables of tiles without a window; 8: tick columns of the debug counters)
  int32_t selfcheck = 0;
  // (_EXCHANGE=0: the tile sums are formed by a pass of their own in front of the summaries, as in round 3)
  int32_t exchange = 1;
  int32_t slots_per_shard = -1;  // _SLOTS_PER_SHARD, tests: run out of slots (tiles then take the chain kernel's
                                 // recompute-from-the-pairs path); absent or negative: as many as the layout wants
  bool repair_on = true;         // (_REPAIR=0: no repair pass in a Fit's first Evaluate -- measurement)
  bool spec_on = true;           // (_SPEC=0: no walk ahead of a wait -- measurement)
};

// ---- the block ---------------------------------------------------------------------------------------------------------
enum StrictRegion : int32_t {  // (the order they lie in)
  kRegTileSum, kRegTileErr, kRegTilePub, kRegTileArrived, kRegTilePairs, kRegRecs, kRegAux, kRegAuxTerms, kRegJobs,
  kRegCand, kRegXyzCaller, kRegCounters, kRegDbg, kRegStamps, kRegChunkState,
  kStrictRegions
};
// inside kRegCounters: the chain kernel's ticket, and the slot counters of the shards, a 128-byte line each
constexpr size_t kDoneRowsAt = 12, kAuxCountAt = 256;

struct StrictLayout {
  struct Span {
    size_t offset, bytes;
  };
  struct Run {  // regions first..last, which lie one behind the other
    int32_t first, last;
  };
  int64_t ntiles = 1, ntiles_pad = 128;
  int32_t nchunks = 1, naux = 0;
  Span region[kStrictRegions] = {};
  size_t total = 0;
  // slot / ticket counters and debug counters start at zero (the chain kernel re-zeroes what it consumed), the arrival
  // bits, the chunks' hand-over words (epoch 0: no launch's); between two Fits: whatever a launch that ended early (a
  // broken ring) left in the counters and the arrival bits
  Run zero_create[3] = {{kRegCounters, kRegDbg}, {kRegTileArrived, kRegTileArrived}, {kRegChunkState, kRegChunkState}};
  Run zero_reset[2] = {{kRegCounters, kRegCounters}, {kRegTileArrived, kRegTileArrived}};
  Span span(Run r) const { return {region[r.first].offset, region[r.last].offset + region[r.last].bytes - region[r.first].offset}; }
};

inline StrictLayout plan_strict_layout(int64_t nt, const StrictKnobs &k, const StrictFacts &f = StrictFacts()) {
  StrictLayout L;
  L.ntiles = nt > 0 ? (nt + f.tile - 1) / f.tile : 1;
  L.ntiles_pad = (L.ntiles + 127) & ~(int64_t)127;
  L.nchunks = (int32_t)((L.ntiles + f.chain_tiles - 1) / f.chain_tiles);
  // slots for the tiles that cross a level or have no window (6 KB of leaf records + 8 KB of terms each):
  // a quarter of all tiles, far more than ever seen (C4: ~2 %; a sum hovering around zero over the whole
  // row: ~15 %); a tile that finds none left is recomputed from the pairs by the chain kernel
  L.naux = (int32_t)(f.aux_shards * ((f.rows * L.ntiles / 4 + f.aux_shards - 1) / f.aux_shards + 4));
  if (k.slots_per_shard >= 0 && (int64_t)k.slots_per_shard * f.aux_shards < L.naux) L.naux = k.slots_per_shard * f.aux_shards;
  const size_t nt1 = (size_t)L.ntiles, na = (size_t)L.naux;
  const int64_t n_groups = (L.ntiles + 31) / 32;
  const auto set = [&L](StrictRegion r, size_t bytes) { L.region[r].bytes = bytes; };
  set(kRegTileSum, (size_t)f.rows * nt1 * sizeof(double));
  set(kRegTileErr, (size_t)f.rows * nt1 * sizeof(double));
  set(kRegTilePub, (size_t)L.ntiles_pad * 16 * sizeof(double));  // (256-byte aligned: a tile's line is one 128-byte line)
  set(kRegTileArrived, (size_t)(n_groups + (n_groups + 31) / 32) * 128);
  set(kRegTilePairs, nt1 * sizeof(uint32_t));
  set(kRegRecs, (size_t)f.rows * nt1 * f.tile_rec);
  set(kRegAux, na * f.lanes * f.leaf_aux);
  set(kRegAuxTerms, na * f.tile * sizeof(float));
  set(kRegJobs, na * f.job_desc);
  set(kRegCand, na * f.cand * sizeof(uint32_t));
  set(kRegXyzCaller, (size_t)(nt ? nt : 1) * 12 + 64);
  set(kRegCounters, kAuxCountAt + (size_t)f.aux_shards * 128);
  set(kRegDbg, 64 * sizeof(unsigned long long));
  set(kRegStamps, nt1 * 16 * sizeof(unsigned long long));
  set(kRegChunkState, (size_t)f.rows * L.nchunks * 16 * sizeof(unsigned long long));
  for (int r = 0; r < kStrictRegions; r++) {
    L.region[r].offset = L.total;
    L.region[r].bytes = (L.region[r].bytes + 255) & ~(size_t)255;
    L.total += L.region[r].bytes;
  }
  return L;
}

// ---- a step's launches ---------------------------------------------------------------------------------------------------
enum StrictForm : int32_t { kOneGpu, kCollective, kRing };  // strict_enqueue, strict_enqueue_sharded, strict_enqueue_ring
enum StrictSummary : int32_t {  // strict_sum_kernel's instantiations
  kSumNone,
  kSumPlain,      // <false>
  kSumExchange,   // <true>
  kSumRing,       // <true, true>
  kSumCertified,  // <true, false, true>: the step's correspondence as well, no grid pass in front (icp.hip)
  kSumCertifyError  // the certified terms need the exchange and the pairs in the caller's order
};
enum StrictChain : int32_t {  // strict_chain_kernel's
  kChainNone,
  kChainCheck,  // <true, false>
  kChainSpec,   // <false, true>: its walkers walk ahead of a wait for their start state
  kChainPlain   // <false, false>
};

struct StrictStep {  // the session's buffers (StrictLayout, StrictWork::nrows) and what the caller says of this step
  int64_t ntiles = 1;
  int32_t nchunks = 1, naux = 0, nrows = 9;
  int32_t rank = 0, world = 1;  // (sharded forms)
  bool have_tile_sums = false;  // one GPU: the correspondence kernel formed them
  bool first_iter = false;      // the first Evaluate of a Fit
  bool certify = false;         // one GPU: CertifiedTerms were given
  bool caller_order = false;    // no pos_of: the pairs are in the caller's order
  bool fuse_update = false;     // one GPU: the chain kernel ends in the pose update
  bool local_failed = false;    // sharded forms: this rank cannot go on
};

struct StrictLaunches {
  bool live = true;  // false, a failed rank: no stage of the step is entered (no kernel below, no ProfScope)
  bool tilesum = false;                  // strict_tilesum_kernel, a workgroup per tile
  int32_t summary = kSumNone;            // a workgroup per tile
  int32_t exchange = 1;                  // StrictWork::exchange as the kernels get it
  bool bases_behind_summary = false;     // row_base / err_base are set behind the summary launch, not before
  uint32_t ring_err_grid = 0;            // strict_ring_err_kernel; 0: does not run
  uint32_t repair_grid = 0, jobs_grid = 0;  // strict_repair_kernel, strict_job_kernel; 0: does not run
  int32_t chain = kChainNone;
  uint32_t chain_grid = 0;
  int32_t fuse_update = 0;
};

inline StrictLaunches plan_strict_launches(StrictForm form, const StrictStep &s, const StrictKnobs &k,
                                           const StrictFacts &f = StrictFacts()) {
  StrictLaunches L;
  // the collective form hands the session's `exchange` to the kernels unchanged although its summaries never exchange;
  // the ring form rides on the summary kernel's own exchange, whatever the session says
  L.exchange = form == kRing ? 1 : k.exchange;
  // A rank that cannot go on launches nothing of the step: in the collective form it keeps calling the collectives with
  // its flag up and launches the base, zero, hop and finish kernels between them (strict_enqueue_sharded), in the ring
  // form it raises the abort word and launches strict_ring_fail_kernel (strict_enqueue_ring).
  if (form != kOneGpu && s.local_failed) {
    L.live = false;
    return L;
  }
  if (form == kOneGpu) {
    L.tilesum = !s.have_tile_sums && !k.exchange;
    L.summary = s.certify ? (k.exchange && s.caller_order ? kSumCertified : kSumCertifyError) : (k.exchange ? kSumExchange : kSumPlain);
    if (L.summary == kSumCertifyError) return L;  // (the step ends there: nothing behind the tile sums runs)
  } else if (form == kCollective) {  // the ranks exchange float64 totals of the tile sums in front of the summaries:
    L.tilesum = true;                // always the pass of its own and <false>, whatever `exchange` says
    L.summary = kSumPlain;
  } else {
    L.summary = kSumRing;
    // this rank's totals of the rounding errors to the ranks behind it; ranks > 0: one workgroup more fetches the totals of
    // the ranks before it, and the job tiles' guesses start from them (row_base, err_base: the summary launch itself
    // finds them unset, as on rank 0)
    L.ring_err_grid = s.world > 1 ? (uint32_t)(f.rows + (s.rank > 0 ? 1 : 0)) : 0u;
    L.bases_behind_summary = s.rank > 0;
  }
  // (the first Evaluate of a Fit: the plain tiles the rows' drift has carried across a binade's end become jobs; never in
  // the collective form)
  if (form != kCollective && s.first_iter && s.naux > 0 && s.ntiles >= f.repair_min_tiles && k.repair_on)
    L.repair_grid = (uint32_t)(s.nrows * ((s.ntiles + f.repair_block - 1) / f.repair_block));
  if (s.naux > 0) L.jobs_grid = (uint32_t)f.job_roles * (uint32_t)s.naux;
  // The chain kernel.  kChainSpec: some walker of THIS launch waits for its start state with spec_depth walks in front of
  // it (several chunks; in the ring form also a rank behind another, which always waits) -- the instantiation with that
  // code spills thirty scalar registers more, which the real walk pays for, 0.7 us a step.  One chunk on one GPU: the
  // kernel without it.  (The collective form's walks go round the ranks between launches: its ranks count as rank 0.)
  const bool waits = form == kRing || s.nchunks > 1;
  const int64_t walks_ahead = (int64_t)(form == kRing ? s.rank : 0) * s.nchunks + s.nchunks - 1;
  L.chain = (k.selfcheck & 1) ? kChainCheck : (waits && k.spec_on && walks_ahead >= k.spec_depth ? kChainSpec : kChainPlain);
  L.chain_grid = (uint32_t)(s.nrows * s.nchunks);
  L.fuse_update = form == kOneGpu ? (s.fuse_update ? 1 : 0) : (form == kRing ? 1 : 0);
  return L;
}

// ---- the block a sharded step exchanges through ([world + 4][16] doubles, StrictBuffers::shard) ----------------------------
struct ShardPlan {
  bool allocate;  // none yet, or one for another world
  bool zero;      // the ring form keeps 32 doubles + a flag word of it; a block the collective form used holds that form's
                  // doubles where the flag word lies -- one equal to this step's number would let tiles read ring_base
                  // before tile 0 wrote it
  size_t bytes;
  bool ring;      // the block is laid out (and zeroed) for the ring form
};
inline ShardPlan plan_shard(bool have_block, int block_world, bool block_ring, int world, bool want_ring) {
  const bool allocate = !have_block || block_world != world;
  return {allocate, want_ring && (allocate || !block_ring), (size_t)(world + 4) * 16 * sizeof(double), want_ring};
}

}  // namespace pcgx
