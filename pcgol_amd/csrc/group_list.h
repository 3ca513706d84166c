// group_list.h -- a grouped id list on the device: what the kernels of group_stats.hip (group geometry) and of
// group_hull.hip (group footprints) share.  The clamps of the contract (include/pcgx.h, "group geometry": G, the sizes,
// the clip at cap_ids), the workgroup's scan, a slot's member, the runs of a wave's row and the wave's carry for
// min / max combines on order-preserving keys.  The offsets' tile sums and the slot -> group map are kernels of
// group_stats.hip; the two launchers at the end enqueue them.
#pragma once
#include "group_terms.h"
#include "range_walk.h"

namespace pcgx {

constexpr int kGsBlock = 256, kGsRow = 64, kGsRowsPerWave = 4;
constexpr int kGsTile = kGsBlock * kGsRowsPerWave;  // slots (and, in the scan, groups) per workgroup
constexpr int kGsGatherRows = 16;                   // rows a wave of the gathers takes one after the other (four tiles a workgroup)
constexpr int kGsGatherTile = kGsBlock / 64 * kGsGatherRows * kGsRow;
static_assert(kGsTile % kGsRow == 0 && kGsRow == 64, "a row is a wave");
static_assert(kGsGatherTile % kGsTile == 0, "the map is made in whole tiles");

// G = clamp(*d_n, 0, cap) read on the device; d_n == nullptr: cap
__device__ __forceinline__ int32_t gs_groups(const int32_t *__restrict__ d_n, const int32_t cap) {
  if (!d_n) return cap;
  const int32_t v = *d_n;
  return v < 0 ? 0 : (v > cap ? cap : v);
}

// the clamped size of entry g of the scan: [0, cap_ids] for a group below G, 0 from G on (entry cap_groups included)
__device__ __forceinline__ uint64_t gs_size_at(const int32_t *__restrict__ sizes, const int64_t g, const int32_t G,
                                               const int32_t cap_ids) {
  if (g >= (int64_t)G) return 0ull;
  const int32_t s = sizes[g];
  return (uint64_t)(s < 0 ? 0 : (s > cap_ids ? cap_ids : s));
}

// exclusive prefix of t over the 256 lanes of the workgroup; total: the workgroup's sum.  All lanes call it.
__device__ __forceinline__ uint64_t gs_block_excl_scan(const uint64_t t, uint64_t *s_w, uint64_t &total) {
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  unsigned long long inc = t;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long v = __shfl_up(inc, o);
    if (lane >= o) inc += v;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint64_t base = 0ull;
  total = 0ull;
#pragma unroll
  for (int w = 0; w < kGsBlock / 64; w++) {
    if (w < wave) base += s_w[w];
    total += s_w[w];
  }
  __syncthreads();  // (s_w may be written again)
  return base + inc - t;
}

// ------------------------------------------------------------------ the gathers
struct GroupList {
  const float4 *nodes;    // the handle's tree, BFS slots
  const uint32_t *inv;    // [n] id -> BFS slot
  int64_t n;              // Len()
  const int32_t *ids;     // [cap_ids]
  const int32_t *grp;     // [whole tiles] slot -> group, -1 behind the list
};

// the slot of this lane in row `row`: its group (or -1) and, for a live member, its coordinates
__device__ __forceinline__ bool gs_member(const GroupList &L, const int64_t slot, int32_t &g, float &x, float &y, float &z) {
  g = L.grp[slot];
  x = y = z = 0.0f;
  if (g < 0) return false;
  const int64_t id = (int64_t)L.ids[slot];  // (g >= 0: the slot is below the list's clipped end, so below cap_ids)
  if (!group_id_ok(id, L.n)) return false;
  const float4 nd = node_at(L.nodes, L.inv[id]);
  x = nd.x;
  y = nd.y;
  z = nd.z;
  return group_point_ok(x, y, z);
}

// is this lane the first of its run (the maximal stretch of one group inside the wave's row)?  All 64 lanes call it.
__device__ __forceinline__ bool gs_run_head(const int32_t g, const int lane) {
  const int32_t prev = __shfl_up(g, 1);
  return lane == 0 || prev != g;
}
// does lane + o belong to this lane's run?  (groups never decrease along a row: the same group means the same run)
__device__ __forceinline__ bool gs_same_run(const int32_t g, const int lane, const int o) {
  const int32_t og = __shfl_down(g, o);
  return lane + o < 64 && og == g;
}

// A wave's carry: rows that belong to one group from end to end are combined in registers (every lane holds the same
// values) and reach memory once when the group changes or the wave is done -- the waves of one large group would
// otherwise send an atomic per row to one address, and same-address atomics are served one after the other
// (radius_graph.h, wave_root_flush: 150k of them took 2 ms).
template <class K>
struct GroupCarry {
  int32_t g;
  K lo[3], hi[3];
  __device__ __forceinline__ void flush(K *__restrict__ keys, const int lane, const K none) {
    if (g >= 0 && lane == 0 && lo[0] != none) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        atomicMin(keys + 6 * (size_t)g + c, lo[c]);
        atomicMax(keys + 6 * (size_t)g + 3 + c, hi[c]);
      }
    }
    g = -1;
  }
};

// One row's keys (lo / hi of this lane's member, the neutral keys for a dead slot) reduced over the runs of the row and
// combined into keys[6 g ..]: a row of one group goes into the carry, the runs of any other row straight to memory.
// All 64 lanes call it.
template <class K>
__device__ __forceinline__ void gs_combine_row(const int32_t g, K (&lo)[3], K (&hi)[3], const int lane, GroupCarry<K> &carry,
                                               K *__restrict__ keys, const K none) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const bool same = gs_same_run(g, lane, o);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const K a = __shfl_down(lo[c], o), b = __shfl_down(hi[c], o);
      if (same) {
        lo[c] = a < lo[c] ? a : lo[c];
        hi[c] = b > hi[c] ? b : hi[c];
      }
    }
  }
  const int32_t g0 = __shfl(g, 0);
  if (__ballot(g != g0) == 0ull) {  // uniform: one group from end to end (g0 >= 0: the row is not behind the list), lane 0 has its keys
    if (carry.g != g0) {
      carry.flush(keys, lane, none);
      carry.g = g0;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        carry.lo[c] = __shfl(lo[c], 0);
        carry.hi[c] = __shfl(hi[c], 0);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const K a = __shfl(lo[c], 0), b = __shfl(hi[c], 0);
        carry.lo[c] = a < carry.lo[c] ? a : carry.lo[c];
        carry.hi[c] = b > carry.hi[c] ? b : carry.hi[c];
      }
    }
    return;
  }
  carry.flush(keys, lane, none);
  const bool head = gs_run_head(g, lane);
  if (head && g >= 0 && lo[0] != none) {  // (no value's key is all ones: the run has a live member)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      atomicMin(keys + 6 * (size_t)g + c, lo[c]);
      atomicMax(keys + 6 * (size_t)g + 3 + c, hi[c]);
    }
  }
}

// group_stats.hip: the tile sums of the clamped sizes (cap_groups + 1 entries, kGsTile to a tile) and their exclusive
// scan, in place: what an offsets kernel starts from
void group_scan_launch(const int32_t *d_sizes, const int32_t *d_n_groups, int32_t cap_groups, int32_t cap_ids,
                       uint64_t *tile_sum, unsigned scan_tiles, hipStream_t st);
// ... and grp[slot] = the slot's group (-1 from the list's clipped end on) over slot_tiles whole tiles, from the offsets
void group_map_launch(const int32_t *off, const int32_t *d_n_groups, int32_t cap_groups, int32_t *grp, unsigned slot_tiles,
                      hipStream_t st);
// ... and group geometry itself for a caller inside a call of its own (planes.hip): centroid [3], eig [3] and axes [9]
// per group, the bits pcgx_kdtree_group_stats_dev gives; Len() > 0, cap_groups > 0; the temporaries come from
// ctx().arena WITHOUT restarting it
pcgx_status group_frames_enqueue(const pcgx_kdtree *t, const int32_t *d_ids, int64_t cap_ids, const int32_t *d_sizes,
                                 int64_t cap_groups, double *d_centroid, double *d_eig, double *d_axes, hipStream_t st);

}  // namespace pcgx
