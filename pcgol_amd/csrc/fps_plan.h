// What pcgx_kdtree_fps_dev (fps.hip) allocates and launches, decided in one place: plan_fps() says how the points are
// cut into tiles, how many tiles a workgroup of the pick kernel takes, how many pick launches a call enqueues and the
// size of every temporary.  Plain C++ on host values: no HIP, no environment, no handle -- fps.hip allocates from the
// arena and enqueues what the plan says; tests/test_fps_plan.py compiles this header with g++ and walks the plan over
// its input space.  (Every pick runs WIDE, one launch over all tiles.  A one-workgroup form for runs
// of late picks was built and measured against this one; it lost at 1M points and was taken out, DESIGN.md 3.28, so the
// plan has no split and no knob to decide.)
#pragma once
#include <cstddef>
#include <cstdint>

namespace pcgx {

// the kernels' constants the plan depends on (fps.hip static_asserts them against its own)
struct FpsFacts {
  int32_t tile = 256;             // kFpsTile: points of a tile, four per lane of the wave that takes it
  int32_t waves = 4;              // waves of a pick workgroup: it takes a multiple of this many tiles
  int32_t wave = 64;              // lanes of a wave: a lane tests one tile's bound, so a wave takes at most this many
  int64_t max_workgroups = 256;   // of one pick launch (a workgroup per CU): beyond it a workgroup takes more tiles,
                                  // up to waves * wave, and beyond that the launch grows after all
};

enum FpsBuf : int32_t {
  kFpsBufXyz,    // float [3 n]: the points by id, NaN where the handle has none (deleted)
  kFpsBufPerm,   // int32 [n]: position -> id, the Morton order
  kFpsBufRec,    // float4 [n]: {x, y, z, bits(id)} by position
  kFpsBufDist,   // float [n]: d by position
  kFpsBufOwner,  // int32 [n]: the owning pick's POSITION in the pick order, by position
  kFpsBufCand,   // uint8 [n]: 1 a candidate, 0 picked or not eligible, by position
  kFpsBufPos,    // uint32 [n]: id -> position
  kFpsBufBox,    // float4 [2 tiles]: the tiles' boxes over their eligible members
  kFpsBufKey,    // uint64 [tiles]: the largest key among a tile's candidates
  kFpsBufBest,   // uint64 [picks + 1]: best[j] = the key of pick j; best[picks] = what the next pick would have been
  kFpsBufs
};

struct FpsPlan {
  int64_t picks = 0;       // pick launches: min(count, n) -- there are no more points than n to pick
  int32_t tile = 0;        // points per tile
  int64_t tiles = 0;       // ceil(n / tile)
  int32_t wg_tiles = 0;    // tiles per workgroup of a pick launch (a multiple of the workgroup's waves)
  int64_t workgroups = 0;  // ceil(tiles / wg_tiles)
  size_t bytes[kFpsBufs] = {};
};

inline FpsPlan plan_fps(const int64_t n, const int64_t count, const FpsFacts &f = FpsFacts()) {
  FpsPlan p;
  if (n <= 0 || count <= 0) return p;
  p.picks = count < n ? count : n;
  p.tile = f.tile;
  p.tiles = (n + f.tile - 1) / f.tile;
  int64_t w = f.waves;
  while ((p.tiles + w - 1) / w > f.max_workgroups && 2 * w <= (int64_t)f.waves * f.wave) w *= 2;
  p.wg_tiles = (int32_t)w;
  p.workgroups = (p.tiles + w - 1) / w;
  const size_t un = (size_t)n, ut = (size_t)p.tiles;
  p.bytes[kFpsBufXyz] = un * 12;
  p.bytes[kFpsBufPerm] = un * 4;
  p.bytes[kFpsBufRec] = un * 16;
  p.bytes[kFpsBufDist] = un * 4;
  p.bytes[kFpsBufOwner] = un * 4;
  p.bytes[kFpsBufCand] = un;
  p.bytes[kFpsBufPos] = un * 4;
  p.bytes[kFpsBufBox] = ut * 32;
  p.bytes[kFpsBufKey] = ut * 8;
  p.bytes[kFpsBufBest] = ((size_t)p.picks + 1) * 8;
  return p;
}

}  // namespace pcgx
