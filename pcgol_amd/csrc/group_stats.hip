// group_stats.hip -- per-group geometry of a tree's points, grouped: count, box, centroid, covariance, principal frame and
// oriented box of every group of a grouped id list (extension: no reference parity; include/pcgx.h, "group geometry").
//
// The list is what pcgx_kdtree_clusters writes (ids cluster by cluster, sizes, a count on the device), and what region
// growing's components, a plane's inliers or a keypoint list are.  Group sizes range from 1 to Len() in one call -- one
// large cluster beside 10^5 singletons is the normal LiDAR case -- so the work is dealt by SLOTS of the list, not by
// groups.  Stages, all on the caller's stream, no count known to the host:
//   offsets   an exclusive scan of the clamped sizes (tile sums, one block over the tile sums, the tiles again), the
//             offsets saturated at cap_ids: the list is clipped there.
//   map       slot -> group.  A tile of kGsTile slots finds the groups of its first and last slot by bisection of the
//             offsets, puts the heads of the groups that start inside it into LDS and max-scans them.
//   box       a gather of xyz by id through the handle's id -> node map; a wave takes kGsRow consecutive slots at a time
//             (a row), reduces min / max over each maximal run of one group inside the row by a segmented shuffle
//             reduction on order-preserving keys (group_terms.h), and the run's first lane combines into the group's row
//             with integer atomics.  Rows that are one group from end to end are first combined in the wave's registers
//             over its kGsGatherRows rows: a large group sends one combine per wave, not one per row, to its address.
//   moments   the second gather: count and nine float64 sums centred on the group's pivot (the centre of its box),
//             reduced over the same runs; the run of group g in row r writes ONE record to slot r + g of an array of
//             rows + cap_groups records.  r + g rises strictly from one run to the next, so no two runs share a slot.
//   frames    a lane per group adds the group's records in row order (a group of more than kGsLaneRows rows: the whole
//             wave, lanes striding the rows, then a butterfly whose shape depends on nothing but the row count), forms
//             centroid and covariance, runs cov3.h's Jacobi with A and V in registers and orders and signs the axes.
//   extents   the third gather: the projections on the three axes in float64, min / max per run, combined as the box is.
//   boxes     a lane per group writes the oriented box.
// Every row of [0, cap_groups) of every output is written on every call.  Integer atomics only, no floating-point
// atomic feeds a sum: the same input gives the same bits on every call.
#include <math.h>
#include <stdlib.h>

#include "group_list.h"

namespace pcgx {

constexpr int kGsLaneRows = 4;                      // a group of up to this many rows is summed by its own lane
constexpr int kGsRec = 10;                          // doubles per record: nine sums and the count

// ------------------------------------------------------------------ offsets
// entries: cap_groups + 1 (the last one is the total's place), kGsTile to a workgroup, four consecutive ones to a lane
__global__ __launch_bounds__(kGsBlock) void gs_tile_sum_kernel(const int32_t *__restrict__ sizes,
                                                               const int32_t *__restrict__ d_n, int32_t cap_groups,
                                                               int32_t cap_ids, uint64_t *__restrict__ tile_sum) {
  __shared__ uint64_t s_w[kGsBlock / 64];
  const int32_t G = gs_groups(d_n, cap_groups);
  const int64_t g0 = (int64_t)blockIdx.x * kGsTile + 4 * (int64_t)threadIdx.x;
  uint64_t t = 0ull;
#pragma unroll
  for (int k = 0; k < 4; k++) t += gs_size_at(sizes, g0 + k, G, cap_ids);
  uint64_t total;
  gs_block_excl_scan(t, s_w, total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one workgroup: tile_sum[0 .. nt) -> its exclusive prefix, in place
__global__ __launch_bounds__(kGsBlock) void gs_tile_scan_kernel(uint64_t *__restrict__ tile_sum, int32_t nt) {
  __shared__ uint64_t s_w[kGsBlock / 64];
  uint64_t carry = 0ull;
  for (int32_t b = 0; b < nt; b += kGsBlock) {  // uniform
    const int32_t i = b + (int32_t)threadIdx.x;
    const uint64_t v = i < nt ? tile_sum[i] : 0ull;
    uint64_t total;
    const uint64_t ex = gs_block_excl_scan(v, s_w, total);
    if (i < nt) tile_sum[i] = carry + ex;
    carry += total;
  }
}

// off[g] = min(sum of the clamped sizes before g, cap_ids) for g in [0, cap_groups]; and the keys the min / max combines
// of the call start from
__global__ __launch_bounds__(kGsBlock) void gs_offsets_kernel(const int32_t *__restrict__ sizes,
                                                              const int32_t *__restrict__ d_n, int32_t cap_groups,
                                                              int32_t cap_ids, const uint64_t *__restrict__ tile_base,
                                                              int32_t *__restrict__ off, uint32_t *__restrict__ box,
                                                              unsigned long long *__restrict__ ext) {
  __shared__ uint64_t s_w[kGsBlock / 64];
  const int32_t G = gs_groups(d_n, cap_groups);
  const int64_t g0 = (int64_t)blockIdx.x * kGsTile + 4 * (int64_t)threadIdx.x;
  uint64_t v[4], t = 0ull;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    v[k] = gs_size_at(sizes, g0 + k, G, cap_ids);
    t += v[k];
  }
  uint64_t total;
  uint64_t at = tile_base[blockIdx.x] + gs_block_excl_scan(t, s_w, total);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int64_t g = g0 + k;
    if (g <= (int64_t)cap_groups) off[g] = (int32_t)(at < (uint64_t)cap_ids ? at : (uint64_t)cap_ids);
    if (g < (int64_t)cap_groups) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        box[6 * g + c] = kGroupKeyMin32;
        box[6 * g + 3 + c] = kGroupKeyMax32;
        ext[6 * g + c] = kGroupKeyMin64;
        ext[6 * g + 3 + c] = kGroupKeyMax64;
      }
    }
    at += v[k];
  }
}

// ------------------------------------------------------------------ map
// the largest g in [0, G) with off[g] <= s, for a slot s < off[G] (so G >= 1): the group that owns the slot
__device__ __forceinline__ int32_t gs_group_of(const int32_t *__restrict__ off, const int32_t G, const int32_t s) {
  int32_t lo = 0, hi = G;  // off[lo] <= s < off[hi]
  while (hi - lo > 1) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= s) lo = mid;
    else hi = mid;
  }
  return lo;
}

// grp[slot] = the slot's group, -1 from the list's (clipped) end on; grp holds whole tiles
__global__ __launch_bounds__(kGsBlock) void gs_map_kernel(const int32_t *__restrict__ off, const int32_t *__restrict__ d_n,
                                                          int32_t cap_groups, int32_t *__restrict__ grp) {
  __shared__ int32_t s_head[kGsTile];
  __shared__ int32_t s_w[kGsBlock / 64];
  const int32_t G = gs_groups(d_n, cap_groups);
  const int64_t lo = (int64_t)blockIdx.x * kGsTile;
  const int64_t total = (int64_t)off[G];
#pragma unroll
  for (int k = 0; k < kGsRowsPerWave; k++) s_head[threadIdx.x + kGsBlock * k] = -1;
  __syncthreads();
  if (lo < total) {  // uniform
    const int64_t last = (lo + kGsTile < total ? lo + kGsTile : total) - 1;
    const int32_t g_lo = gs_group_of(off, G, (int32_t)lo), g_hi = gs_group_of(off, G, (int32_t)last);
    if (threadIdx.x == 0) s_head[0] = g_lo;
    // the groups behind g_lo up to g_hi start inside the tile; an empty one shares its offset with the next and owns nothing
    for (int64_t g = (int64_t)g_lo + 1 + threadIdx.x; g <= (int64_t)g_hi; g += kGsBlock) {
      const int32_t o = off[g];
      if (off[g + 1] > o) s_head[(int64_t)o - lo] = (int32_t)g;
    }
  }
  __syncthreads();
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  int32_t m[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int32_t h = s_head[4 * threadIdx.x + k];
    m[k] = k == 0 ? h : (h > m[k - 1] ? h : m[k - 1]);
  }
  int32_t inc = m[3];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t v = __shfl_up(inc, o);
    if (lane >= o && v > inc) inc = v;
  }
  if (lane == 63) s_w[wave] = inc;
  int32_t before = __shfl_up(inc, 1);
  if (lane == 0) before = -1;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kGsBlock / 64; w++)
    if (w < wave && s_w[w] > before) before = s_w[w];
  int4 out;
  int32_t *o4 = reinterpret_cast<int32_t *>(&out);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int64_t slot = lo + 4 * (int64_t)threadIdx.x + k;
    o4[k] = slot < total ? (m[k] > before ? m[k] : before) : -1;
  }
  *reinterpret_cast<int4 *>(grp + lo + 4 * (int64_t)threadIdx.x) = out;
}

// ------------------------------------------------------------------ the gathers (GroupList, the runs, the carry: group_list.h)
__global__ __launch_bounds__(kGsBlock) void gs_box_kernel(GroupList L, uint32_t *__restrict__ box) {
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  GroupCarry<uint32_t> carry;
  carry.g = -1;
#pragma unroll 1
  for (int k = 0; k < kGsGatherRows; k++) {
    const int64_t row = ((int64_t)blockIdx.x * (kGsBlock / 64) + wave) * kGsGatherRows + k;
    int32_t g;
    float x, y, z;
    const bool live = gs_member(L, row * kGsRow + lane, g, x, y, z);
    if (__ballot(g >= 0) == 0ull) break;  // uniform: the list ended (the groups of later rows are -1 too)
    uint32_t lo[3], hi[3];
    lo[0] = live ? group_key_f32(x) : kGroupKeyMin32;
    lo[1] = live ? group_key_f32(y) : kGroupKeyMin32;
    lo[2] = live ? group_key_f32(z) : kGroupKeyMin32;
    hi[0] = live ? group_key_f32(x) : kGroupKeyMax32;
    hi[1] = live ? group_key_f32(y) : kGroupKeyMax32;
    hi[2] = live ? group_key_f32(z) : kGroupKeyMax32;
    gs_combine_row(g, lo, hi, lane, carry, box, kGroupKeyMin32);
  }
  carry.flush(box, lane, kGroupKeyMin32);
}

__global__ __launch_bounds__(kGsBlock) void gs_moment_kernel(GroupList L, const uint32_t *__restrict__ box,
                                                             double *__restrict__ rec) {
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
#pragma unroll 1
  for (int k = 0; k < kGsGatherRows; k++) {
    const int64_t row = ((int64_t)blockIdx.x * (kGsBlock / 64) + wave) * kGsGatherRows + k;
    int32_t g;
    float x, y, z;
    const bool live = gs_member(L, row * kGsRow + lane, g, x, y, z);
    if (__ballot(g >= 0) == 0ull) break;  // uniform
    GroupSums a;
    a.clear();
    if (live) {
      const uint32_t *b = box + 6 * (size_t)g;
      a.add((double)x - group_pivot(group_unkey_f32(b[0]), group_unkey_f32(b[3])),
            (double)y - group_pivot(group_unkey_f32(b[1]), group_unkey_f32(b[4])),
            (double)z - group_pivot(group_unkey_f32(b[2]), group_unkey_f32(b[5])));
    }
    int32_t cnt = live ? 1 : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const bool same = gs_same_run(g, lane, o);
      GroupSums p;
      p.sx = __shfl_down(a.sx, o);
      p.sy = __shfl_down(a.sy, o);
      p.sz = __shfl_down(a.sz, o);
      p.sxx = __shfl_down(a.sxx, o);
      p.sxy = __shfl_down(a.sxy, o);
      p.sxz = __shfl_down(a.sxz, o);
      p.syy = __shfl_down(a.syy, o);
      p.syz = __shfl_down(a.syz, o);
      p.szz = __shfl_down(a.szz, o);
      p.n = 0;
      const int32_t pc = __shfl_down(cnt, o);
      if (same) {
        a.merge(p);
        cnt += pc;
      }
    }
    const bool head = gs_run_head(g, lane);
    if (head && g >= 0) {  // every run writes its record, a run without a live member zeros: the frames pass reads it
      double *r = rec + (size_t)kGsRec * (size_t)(row + (int64_t)g);
      r[0] = a.sx; r[1] = a.sy; r[2] = a.sz;
      r[3] = a.sxx; r[4] = a.sxy; r[5] = a.sxz; r[6] = a.syy; r[7] = a.syz; r[8] = a.szz;
      r[9] = (double)cnt;
    }
  }
}

// ------------------------------------------------------------------ frames
struct GroupOut {
  int32_t *count;    // [cap_groups]
  float *aabb;       // [6 cap_groups]
  double *centroid;  // [3 cap_groups]
  double *cov;       // [6 cap_groups]
  double *eig;       // [3 cap_groups]
  double *axes;      // [9 cap_groups]
  double *obb;       // [6 cap_groups]
};

__device__ __forceinline__ void gs_add_record(GroupSums &a, const double *__restrict__ r) {
  a.sx += r[0]; a.sy += r[1]; a.sz += r[2];
  a.sxx += r[3]; a.sxy += r[4]; a.sxz += r[5]; a.syy += r[6]; a.syz += r[7]; a.szz += r[8];
  a.n += (int64_t)r[9];
}

// a lane per row g of [0, cap_groups); frame[12 g ..] = centroid and axes, cnt[g] = the count, for the extents
__global__ __launch_bounds__(kGsBlock) void gs_frame_kernel(const int32_t *__restrict__ off, const int32_t *__restrict__ d_n,
                                                            int32_t cap_groups, const uint32_t *__restrict__ box,
                                                            const double *__restrict__ rec, GroupOut O,
                                                            double *__restrict__ frame, int32_t *__restrict__ cnt) {
  const int lane = (int)(threadIdx.x & 63u);
  const int32_t G = gs_groups(d_n, cap_groups);
  const int64_t g = (int64_t)blockIdx.x * kGsBlock + threadIdx.x;
  int32_t o0 = 0, o1 = 0;
  if (g < (int64_t)G) {
    o0 = off[g];
    o1 = off[g + 1];
  }
  const bool owns = o1 > o0;
  const int32_t r0 = o0 >> 6, nr = owns ? ((o1 - 1) >> 6) - r0 + 1 : 0;
  GroupSums a;
  a.clear();
  if (owns && nr <= kGsLaneRows)
    for (int32_t r = 0; r < nr; r++) gs_add_record(a, rec + (size_t)kGsRec * (size_t)((int64_t)r0 + r + g));
  unsigned long long todo = __ballot(owns && nr > kGsLaneRows);
  while (todo) {  // uniform: the wave sums the records of one long group
    const int leader = __ffsll((long long)todo) - 1;
    const int64_t lg = (int64_t)__shfl((int32_t)g, leader);  // (g < 2^31 wherever a group owns slots)
    const int32_t lr0 = __shfl(r0, leader), lnr = __shfl(nr, leader);
    GroupSums p;
    p.clear();
    for (int32_t r = lane; r < lnr; r += 64) gs_add_record(p, rec + (size_t)kGsRec * (size_t)((int64_t)lr0 + r + lg));
    int32_t pn = (int32_t)p.n;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      p.sx += __shfl_xor(p.sx, m);
      p.sy += __shfl_xor(p.sy, m);
      p.sz += __shfl_xor(p.sz, m);
      p.sxx += __shfl_xor(p.sxx, m);
      p.sxy += __shfl_xor(p.sxy, m);
      p.sxz += __shfl_xor(p.sxz, m);
      p.syy += __shfl_xor(p.syy, m);
      p.syz += __shfl_xor(p.syz, m);
      p.szz += __shfl_xor(p.szz, m);
      pn += __shfl_xor(pn, m);
    }
    p.n = pn;
    if (lane == leader) a = p;
    todo &= todo - 1ull;
  }
  if (g >= (int64_t)cap_groups) return;
  const bool any = a.n > 0;
  double c[3] = {0.0, 0.0, 0.0}, cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, eig[3] = {0.0, 0.0, 0.0};
  double ax[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  float bb[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (any) {
    const uint32_t *b = box + 6 * (size_t)g;
#pragma unroll
    for (int k = 0; k < 6; k++) bb[k] = group_unkey_f32(b[k]);
    group_finish(a, group_pivot(bb[0], bb[3]), group_pivot(bb[1], bb[4]), group_pivot(bb[2], bb[5]), c, cov);
    group_frame(cov, eig, ax);
  }
  cnt[g] = (int32_t)a.n;
#pragma unroll
  for (int k = 0; k < 3; k++) frame[12 * (size_t)g + k] = c[k];
#pragma unroll
  for (int k = 0; k < 9; k++) frame[12 * (size_t)g + 3 + k] = ax[k];
  if (O.count) O.count[g] = (int32_t)a.n;
  if (O.aabb)
#pragma unroll
    for (int k = 0; k < 6; k++) O.aabb[6 * (size_t)g + k] = bb[k];
  if (O.centroid)
#pragma unroll
    for (int k = 0; k < 3; k++) O.centroid[3 * (size_t)g + k] = c[k];
  if (O.cov)
#pragma unroll
    for (int k = 0; k < 6; k++) O.cov[6 * (size_t)g + k] = cov[k];
  if (O.eig)
#pragma unroll
    for (int k = 0; k < 3; k++) O.eig[3 * (size_t)g + k] = eig[k];
  if (O.axes)
#pragma unroll
    for (int k = 0; k < 9; k++) O.axes[9 * (size_t)g + k] = ax[k];
}

// ------------------------------------------------------------------ extents and boxes
__global__ __launch_bounds__(kGsBlock) void gs_extent_kernel(GroupList L, const double *__restrict__ frame,
                                                             unsigned long long *__restrict__ ext) {
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  GroupCarry<unsigned long long> carry;
  carry.g = -1;
#pragma unroll 1
  for (int k = 0; k < kGsGatherRows; k++) {
    const int64_t row = ((int64_t)blockIdx.x * (kGsBlock / 64) + wave) * kGsGatherRows + k;
    int32_t g;
    float x, y, z;
    const bool live = gs_member(L, row * kGsRow + lane, g, x, y, z);
    if (__ballot(g >= 0) == 0ull) break;  // uniform
    unsigned long long lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      lo[c] = kGroupKeyMin64;
      hi[c] = kGroupKeyMax64;
    }
    if (live) {
      const double *f = frame + 12 * (size_t)g;
      const double cen[3] = {f[0], f[1], f[2]};
#pragma unroll
      for (int c = 0; c < 3; c++)
        lo[c] = hi[c] = group_key_f64(group_extent(x, y, z, cen, f[3 + 3 * c], f[4 + 3 * c], f[5 + 3 * c]));
    }
    // (all ones is a NaN's key: no extent of a live member of a finite frame)
    gs_combine_row(g, lo, hi, lane, carry, ext, (unsigned long long)kGroupKeyMin64);
  }
  carry.flush(ext, lane, (unsigned long long)kGroupKeyMin64);
}

__global__ __launch_bounds__(kGsBlock) void gs_obb_kernel(int32_t cap_groups, const int32_t *__restrict__ cnt,
                                                          const double *__restrict__ frame,
                                                          const unsigned long long *__restrict__ ext,
                                                          double *__restrict__ obb) {
  const int64_t g = (int64_t)blockIdx.x * kGsBlock + threadIdx.x;
  if (g >= (int64_t)cap_groups) return;
  double out[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const unsigned long long *e = ext + 6 * (size_t)g;
  if (cnt[g] > 0 && e[0] != kGroupKeyMin64) {
    const double *f = frame + 12 * (size_t)g;
    const double c[3] = {f[0], f[1], f[2]};
    const double ax[9] = {f[3], f[4], f[5], f[6], f[7], f[8], f[9], f[10], f[11]};
    const double lo[3] = {group_unkey_f64(e[0]), group_unkey_f64(e[1]), group_unkey_f64(e[2])};
    const double hi[3] = {group_unkey_f64(e[3]), group_unkey_f64(e[4]), group_unkey_f64(e[5])};
    group_obb(c, ax, lo, hi, out);
  }
#pragma unroll
  for (int k = 0; k < 6; k++) obb[6 * (size_t)g + k] = out[k];
}

// ------------------------------------------------------------------ the call
void group_scan_launch(const int32_t *d_sizes, const int32_t *d_n_groups, int32_t cap_groups, int32_t cap_ids,
                       uint64_t *tile_sum, unsigned scan_tiles, hipStream_t st) {
  hipLaunchKernelGGL(gs_tile_sum_kernel, dim3(scan_tiles), dim3(kGsBlock), 0, st, d_sizes, d_n_groups, cap_groups, cap_ids,
                     tile_sum);
  hipLaunchKernelGGL(gs_tile_scan_kernel, dim3(1), dim3(kGsBlock), 0, st, tile_sum, (int32_t)scan_tiles);
}

void group_map_launch(const int32_t *off, const int32_t *d_n_groups, int32_t cap_groups, int32_t *grp, unsigned slot_tiles,
                      hipStream_t st) {
  hipLaunchKernelGGL(gs_map_kernel, dim3(slot_tiles), dim3(kGsBlock), 0, st, off, d_n_groups, cap_groups, grp);
}

static pcgx_status gs_zero_outputs(const GroupOut &O, int64_t cap_groups, hipStream_t st) {
  const size_t c = (size_t)cap_groups;
  if (O.count) PCGX_HIP_TRY(hipMemsetAsync(O.count, 0, c * 4, st));
  if (O.aabb) PCGX_HIP_TRY(hipMemsetAsync(O.aabb, 0, c * 24, st));
  if (O.centroid) PCGX_HIP_TRY(hipMemsetAsync(O.centroid, 0, c * 24, st));
  if (O.cov) PCGX_HIP_TRY(hipMemsetAsync(O.cov, 0, c * 48, st));
  if (O.eig) PCGX_HIP_TRY(hipMemsetAsync(O.eig, 0, c * 24, st));
  if (O.axes) PCGX_HIP_TRY(hipMemsetAsync(O.axes, 0, c * 72, st));
  if (O.obb) PCGX_HIP_TRY(hipMemsetAsync(O.obb, 0, c * 48, st));
  return PCGX_OK;
}

// Len() > 0, cap_groups > 0, everything device resident; temporaries from ctx().arena
static pcgx_status group_stats_enqueue(const pcgx_kdtree *t, const int32_t *d_ids, int64_t cap_ids, const int32_t *d_sizes,
                                       int64_t cap_groups, const int32_t *d_n_groups, const GroupOut &O, hipStream_t st,
                                       bool restart = true) {
  Arena &ar = ctx().arena;
  if (restart) PCGX_TRY(ar.begin(st));
  const uint32_t *inv = nullptr;
  PCGX_TRY(range_inverse_map(t, &inv, st));
  const int64_t entries = cap_groups + 1;
  const unsigned scan_tiles = (unsigned)((entries + kGsTile - 1) / kGsTile);
  const unsigned gather_tiles = (unsigned)((cap_ids + kGsGatherTile - 1) / kGsGatherTile);
  const unsigned slot_tiles = gather_tiles * (kGsGatherTile / kGsTile);  // (the map covers what the gathers read)
  const unsigned group_blocks = (unsigned)((cap_groups + kGsBlock - 1) / kGsBlock);
  const int64_t rows = (int64_t)slot_tiles * (kGsTile / kGsRow);
  uint64_t *tile_sum = nullptr;
  int32_t *off = nullptr, *grp = nullptr, *cnt = nullptr;
  uint32_t *box = nullptr;
  unsigned long long *ext = nullptr;
  double *rec = nullptr, *frame = nullptr;
  PCGX_TRY(ar.alloc_n((size_t)scan_tiles, &tile_sum));
  PCGX_TRY(ar.alloc_n((size_t)entries, &off));
  PCGX_TRY(ar.alloc_n((size_t)slot_tiles * kGsTile + 4, &grp));
  PCGX_TRY(ar.alloc_n((size_t)cap_groups, &cnt));
  PCGX_TRY(ar.alloc_n((size_t)cap_groups * 6, &box));
  PCGX_TRY(ar.alloc_n((size_t)cap_groups * 6, &ext));
  PCGX_TRY(ar.alloc_n((size_t)(rows + cap_groups) * kGsRec, &rec));
  PCGX_TRY(ar.alloc_n((size_t)cap_groups * 12, &frame));
  const int32_t cg = (int32_t)cap_groups, ci = (int32_t)cap_ids;
  group_scan_launch(d_sizes, d_n_groups, cg, ci, tile_sum, scan_tiles, st);
  hipLaunchKernelGGL(gs_offsets_kernel, dim3(scan_tiles), dim3(kGsBlock), 0, st, d_sizes, d_n_groups, cg, ci,
                     (const uint64_t *)tile_sum, off, box, ext);
  const GroupList L{t->d_nodes, inv, t->n, d_ids, grp};
  if (slot_tiles) {
    group_map_launch(off, d_n_groups, cg, grp, slot_tiles, st);
    hipLaunchKernelGGL(gs_box_kernel, dim3(gather_tiles), dim3(kGsBlock), 0, st, L, box);
    hipLaunchKernelGGL(gs_moment_kernel, dim3(gather_tiles), dim3(kGsBlock), 0, st, L, (const uint32_t *)box, rec);
  }
  hipLaunchKernelGGL(gs_frame_kernel, dim3(group_blocks), dim3(kGsBlock), 0, st, (const int32_t *)off, d_n_groups, cg,
                     (const uint32_t *)box, (const double *)rec, O, frame, cnt);
  if (O.obb) {
    if (slot_tiles)
      hipLaunchKernelGGL(gs_extent_kernel, dim3(gather_tiles), dim3(kGsBlock), 0, st, L, (const double *)frame, ext);
    hipLaunchKernelGGL(gs_obb_kernel, dim3(group_blocks), dim3(kGsBlock), 0, st, cg, (const int32_t *)cnt,
                       (const double *)frame, (const unsigned long long *)ext, O.obb);
  }
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

pcgx_status group_frames_enqueue(const pcgx_kdtree *t, const int32_t *d_ids, int64_t cap_ids, const int32_t *d_sizes,
                                 int64_t cap_groups, double *d_centroid, double *d_eig, double *d_axes, hipStream_t st) {
  const GroupOut O{nullptr, nullptr, d_centroid, nullptr, d_eig, d_axes, nullptr};
  return group_stats_enqueue(t, d_ids, cap_ids, d_sizes, cap_groups, nullptr, O, st, false);
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kGroupMax = 0x7fffffff;  // slots, groups and ids are int32 on the device

pcgx_status group_stats_check(const char *fn, const pcgx_kdtree *t, const void *ids, int64_t n_ids, const void *sizes,
                              int64_t n_groups) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (n_ids < 0 || n_groups < 0) return fail(PCGX_E_INVALID, "%s: negative number of ids or groups", fn);
  if (n_ids > kGroupMax || n_groups > kGroupMax || t->n > kGroupMax)
    return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 slots, groups or points", fn);
  if (n_ids > 0 && !ids) return fail(PCGX_E_INVALID, "%s: NULL ids", fn);
  if (n_groups > 0 && !sizes) return fail(PCGX_E_INVALID, "%s: NULL sizes", fn);
  return PCGX_OK;
}

}  // namespace

extern "C" int32_t pcgx_group_stats_tile(void) { return kGsTile; }

extern "C" pcgx_status pcgx_kdtree_group_stats_dev(const pcgx_kdtree *t, const int32_t *d_ids, int64_t cap_ids,
                                                   const int32_t *d_sizes, int64_t cap_groups, const int32_t *d_n_groups,
                                                   int32_t *d_count, float *d_aabb, double *d_centroid, double *d_cov,
                                                   double *d_eig, double *d_axes, double *d_obb, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(group_stats_check("pcgx_kdtree_group_stats_dev", t, d_ids, cap_ids, d_sizes, cap_groups));
  if (cap_groups == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  const GroupOut O{d_count, d_aabb, d_centroid, d_cov, d_eig, d_axes, d_obb};
  if (t->n == 0) return gs_zero_outputs(O, cap_groups, st);  // no point: every slot is dead
  return group_stats_enqueue(t, d_ids, cap_ids, d_sizes, cap_groups, d_n_groups, O, st);
}

extern "C" pcgx_status pcgx_kdtree_group_stats(const pcgx_kdtree *t, const int64_t *ids, int64_t n_ids,
                                               const int64_t *sizes, int64_t n_groups, int64_t *count, float *aabb,
                                               double *centroid, double *cov, double *eig, double *axes, double *obb) {
  PCGX_API_CALL();
  PCGX_TRY(group_stats_check("pcgx_kdtree_group_stats", t, ids, n_ids, sizes, n_groups));
  if (n_groups == 0) return PCGX_OK;
  const int64_t n = t->n;
  RawVector<int32_t> h((size_t)n_ids + (size_t)n_groups);  // the ids, then the sizes
  for (int64_t s = 0; s < n_ids; s++) {
    if (ids[s] < 0 || ids[s] >= n) return fail(PCGX_E_INVALID, "pcgx_kdtree_group_stats: id out of range");
    h[(size_t)s] = (int32_t)ids[s];
  }
  int64_t sum = 0;
  for (int64_t g = 0; g < n_groups; g++) {
    const int64_t s = sizes[g] < 0 ? 0 : sizes[g];
    if (s > n_ids - sum) return fail(PCGX_E_INVALID, "pcgx_kdtree_group_stats: the sizes add up to more than n_ids");
    sum += s;
    h[(size_t)(n_ids + g)] = (int32_t)s;
  }
  PCGX_TRY(ensure_init());
  // always on the device: the sums and the frames are the kernels', not a host restatement
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  const size_t G = (size_t)n_groups;
  int32_t *d_in = nullptr, *d_count = nullptr;
  float *d_aabb = nullptr;
  double *d_cen = nullptr, *d_cov = nullptr, *d_eig = nullptr, *d_axes = nullptr, *d_obb = nullptr;
  PCGX_TRY(ha.alloc_n(h.size(), &d_in));
  PCGX_TRY(staged_upload(d_in, h.data(), h.size() * 4, st));
  if (centroid) PCGX_TRY(ha.alloc_n(G * 3, &d_cen));
  if (cov) PCGX_TRY(ha.alloc_n(G * 6, &d_cov));
  if (eig) PCGX_TRY(ha.alloc_n(G * 3, &d_eig));
  if (axes) PCGX_TRY(ha.alloc_n(G * 9, &d_axes));
  if (obb) PCGX_TRY(ha.alloc_n(G * 6, &d_obb));
  if (aabb) PCGX_TRY(ha.alloc_n(G * 6, &d_aabb));
  if (count) PCGX_TRY(ha.alloc_n(G, &d_count));
  PCGX_TRY(pcgx_kdtree_group_stats_dev(t, d_in, n_ids, d_in + n_ids, n_groups, nullptr, d_count, d_aabb, d_cen, d_cov, d_eig,
                                       d_axes, d_obb, st));
  if (count) {
    RawVector<int32_t> c(G);
    PCGX_TRY(staged_download(c.data(), d_count, G * 4, st));
    for (size_t g = 0; g < G; g++) count[g] = c[g];
  }
  if (aabb) PCGX_TRY(staged_download(aabb, d_aabb, G * 24, st));
  if (centroid) PCGX_TRY(staged_download(centroid, d_cen, G * 24, st));
  if (cov) PCGX_TRY(staged_download(cov, d_cov, G * 48, st));
  if (eig) PCGX_TRY(staged_download(eig, d_eig, G * 24, st));
  if (axes) PCGX_TRY(staged_download(axes, d_axes, G * 72, st));
  if (obb) PCGX_TRY(staged_download(obb, d_obb, G * 48, st));
  return PCGX_OK;
}
