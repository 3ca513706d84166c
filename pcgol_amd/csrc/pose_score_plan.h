// What pcgx_kdtree_score_poses_dev (pose_score.hip) allocates and launches, decided in one place: plan_score() says which
// path a call takes, how many poses a round of launches scores (the chunk), how many tiles the source has, and the size
// of every temporary.  Plain C++ on host values: no HIP, no environment, no handle -- pose_score.hip reads the handle and
// PCGX_SCORE_CHUNK, allocates from the arena and enqueues what the plan says; tests/test_score_plan.py compiles this
// header with g++ and walks the plan over its input space.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pcgx {

// the kernels' constants the plan depends on (pose_score.hip static_asserts them against its own)
struct ScoreFacts {
  int32_t tile = 256;                    // kScoreTile: source points per workgroup
  int32_t wave = 64;                     // lanes of a wave: one mask word per wave and pose
  int64_t pair_budget = (int64_t)1 << 22;  // pairs a round may leave to the walk: chunk * n stays below this where chunk > 1
  int64_t max_chunk = 65535;             // gridDim.y
  size_t partial_rec = 16;               // sizeof(ScorePartial)
};

enum ScorePath : int32_t {
  kScoreNothing = 0,  // K == 0 or n == 0: counts and sums are zero, only the record is made
  kScoreEmpty = 1,    // every point of the tree was deleted: no pair can be found
  kScoreFused = 2,    // grid enabled, no deletions: score_fused_kernel, the walk for what the grid leaves, score_walk_add_kernel
  kScorePlain = 3,    // deletions, or no grid: per pose transform, the handle's own search, score_count_kernel
};

struct ScoreInputs {
  int64_t n = 0, K = 0;          // source points, poses (both checked: 0 .. 2^31 - 1)
  bool grid = false;             // grid_enabled(t)
  bool deletions = false;        // t->n_deleted > 0
  bool empty = false;            // t->n_deleted == t->n
  int64_t forced_chunk = 0;      // PCGX_SCORE_CHUNK (<= 0: not set)
  size_t sort_workspace = 0;     // radix_sort_workspace_bytes(n)
  bool have_counts = false, have_sums = false;  // the caller gave d_counts / d_sums
};

enum ScoreBuf : int32_t {
  kBufCounts,     // int32 [K] where the caller gave none
  kBufSums,       // float64 [K] where the caller gave none
  kBufBox,        // the source's box: 6 floats
  kBufKeys0, kBufKeys1, kBufVals0, kBufVals1, kBufSortWs,  // the source's order: Morton keys, positions, the sort's workspace
  kBufSrc4,       // float4 [n]: the source in that order
  kBufPartials,   // ScorePartial [chunk * tiles]
  kBufMasks,      // uint64 [chunk * tiles * tile / wave]: which lanes of a wave left their pair to the walk
  kBufWalkQ,      // float [3 * chunk * n]: x' of such a pair, at slot pose-in-chunk * n + position
  kBufWalkList,   // int32 [chunk * n]: the slots in use, in the order they were taken
  kBufWalkIds,    // int32 [chunk * n]: the walk's answers by slot
  kBufWalkDsq,    // float [chunk * n]
  kBufWalkCount,  // uint32 [nchunks]: a round's number of slots in use (a word per round, zeroed once)
  kBufPlainQ,     // float [3 n]: x' of one pose (plain path)
  kBufPlainIds,   // int32 [n]
  kBufPlainDsq,   // float [n]
  kScoreBufs
};

struct ScorePlan {
  int32_t path = kScoreNothing;
  int64_t tiles = 0;    // ceil(n / tile)
  int64_t chunk = 0;    // poses per round; round r scores poses [r * chunk, min(K, (r + 1) * chunk))
  int64_t nchunks = 0;  // rounds
  bool order = false;   // the source is put into Morton order over its own box first
  size_t bytes[kScoreBufs] = {};
};

inline ScorePlan plan_score(const ScoreInputs &in, const ScoreFacts &f = ScoreFacts()) {
  ScorePlan p;
  const int64_t n = in.n, K = in.K;
  const size_t un = (size_t)n, uK = (size_t)K;
  if (!in.have_counts) p.bytes[kBufCounts] = (uK ? uK : 1) * 4;
  if (!in.have_sums) p.bytes[kBufSums] = (uK ? uK : 1) * 8;
  if (n <= 0 || K <= 0) return p;
  if (in.empty) {
    p.path = kScoreEmpty;
    return p;
  }
  p.tiles = (n + f.tile - 1) / f.tile;
  if (in.deletions || !in.grid) {
    p.path = kScorePlain;
    p.chunk = 1;
    p.nchunks = K;
    p.bytes[kBufPartials] = (size_t)p.tiles * f.partial_rec;
    p.bytes[kBufPlainQ] = un * 12;
    p.bytes[kBufPlainIds] = un * 4;
    p.bytes[kBufPlainDsq] = un * 4;
    return p;
  }
  p.path = kScoreFused;
  // the worst case leaves every pair of a round to the walk (a tree of coincident points): chunk * n slots
  int64_t chunk = in.forced_chunk > 0 ? in.forced_chunk : f.pair_budget / n;
  const int64_t slots_max = 0x7fffffffll / n;  // a slot is an int32 (the walk's list)
  if (chunk > slots_max) chunk = slots_max;
  if (chunk > f.max_chunk) chunk = f.max_chunk;
  if (chunk > K) chunk = K;
  if (chunk < 1) chunk = 1;
  p.chunk = chunk;
  p.nchunks = (K + chunk - 1) / chunk;
  p.order = n > 1;
  const size_t slots = (size_t)chunk * un, groups = (size_t)chunk * (size_t)p.tiles;
  if (p.order) {
    p.bytes[kBufBox] = 32;
    p.bytes[kBufKeys0] = p.bytes[kBufKeys1] = p.bytes[kBufVals0] = p.bytes[kBufVals1] = un * 4;
    p.bytes[kBufSortWs] = in.sort_workspace ? in.sort_workspace : 4;
  }
  p.bytes[kBufSrc4] = un * 16;
  p.bytes[kBufPartials] = groups * f.partial_rec;
  p.bytes[kBufMasks] = groups * (size_t)(f.tile / f.wave) * 8;
  p.bytes[kBufWalkQ] = slots * 12;
  p.bytes[kBufWalkList] = p.bytes[kBufWalkIds] = p.bytes[kBufWalkDsq] = slots * 4;
  p.bytes[kBufWalkCount] = (size_t)p.nchunks * 4;
  return p;
}

}  // namespace pcgx
