// group_hull.hip -- per-group footprints of a tree's points, grouped: the exact 2-D convex hull of every group of a
// grouped id list, its area and its minimum-area upright rectangle (extension: no reference parity; include/pcgx.h,
// "group footprints").
//
// One cluster of 10^6 points beside 10^5 singletons is the normal case (group_stats.hip), so the work is dealt by SLOTS
// of the list and then by SURVIVORS, never a group to a lane over all its members.  A member leaves only on exact
// evidence: hull_orient (hull_terms.h) against real input points.  Stages, all on the caller's stream, no count known to
// the host, temporaries from the arena:
//   offsets, map  as group_stats.hip has them (group_list.h).
//   extremes      per group four 64-bit keys by integer atomics with the wave's carry: the lexicographically least and
//                 greatest place (L, R: x then y) and the same with y first (B, T).
//   filter        a slot is classed by the exact side of the line L -> R: below it (class 0, the lower chain; the
//                 places L and R themselves too), above it (class 1, the upper chain), on it strictly between L and R
//                 (no vertex: dropped).  A lower slot strictly left of L -> B and of B -> R lies strictly inside the
//                 triangle L B R and is dropped, an upper one against R -> T and T -> L alike; a zero-length edge or a
//                 triangle of the wrong turn certifies nothing and drops nothing.  Survivors get their sort keys.
//   sort          radix_sort_pairs over the capacity, least significant key first, stable: id, y key, x key, then
//                 2 group + class (dead slots last).  A place's smallest id now stands first among its copies.
//   heads         the first entry of every (group, class, place) is kept: ordered tile compaction (bucket_grid.h).
//   reduce        kGhRounds times: a lane takes kGhChunk consecutive survivors, runs the monotone chain of each stretch of
//                 one (group, class) inside them between the anchors L and R (stack in LDS) and keeps what stays on it;
//                 ordered compaction again.  A survivor that is off the chain of a subset between L and R is off the
//                 group's chain.  Rounds on an empty or unshrinkable list cost a launch each.
//   chain         a lane per group runs the same chain over what is left of its two classes, the stack in global
//                 memory: right for every input, slow where nearly every member is a vertex.
//   finish        the hull sizes are scanned as the sizes were, a lane per group writes the vertices counter-clockwise
//                 from L (lower chain, then the upper one backwards), gh_rect_kernel computes area and rectangle from the
//                 written hulls (a lane per group; a hull of more than 16 vertices by the wave, a lane per edge).
// Integer atomics only; every order is fixed by the input: the same input gives the same bits on every call.
#include <math.h>
#include <stdlib.h>

#include "bucket_grid.h"
#include "group_list.h"
#include "hull_terms.h"

namespace pcgx {

constexpr int kGhChunk = 16;   // survivors a lane of the reduce takes (a 16-byte row of keep flags)
constexpr int kGhRounds = 4;   // reduce rounds before the per-group chain
constexpr uint32_t kGhDead = 0xffffffffu;  // the (group, class) key of a slot that is out

// ------------------------------------------------------------------ offsets
// off[g] = min(sum of the clamped sizes before g, cap_ids) for g in [0, cap_groups]; kInit: and the keys the extremes
// start from (group_stats.hip's gs_offsets_kernel with this file's keys)
template <bool kInit>
__global__ __launch_bounds__(kGsBlock) void gh_offsets_kernel(const int32_t *__restrict__ sizes,
                                                              const int32_t *__restrict__ d_n, int32_t cap_groups,
                                                              int32_t cap_ids, const uint64_t *__restrict__ tile_base,
                                                              int32_t *__restrict__ off,
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
    if (kInit && g < (int64_t)cap_groups) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        ext[6 * g + c] = kGroupKeyMin64;
        ext[6 * g + 3 + c] = kGroupKeyMax64;
      }
    }
    at += v[k];
  }
}

// ------------------------------------------------------------------ extremes
// ext[6 g ..] = the least (x, y) key, the least (y, x) key, (the first again); then the greatest ones: L, B, R, T
__global__ __launch_bounds__(kGsBlock) void gh_extreme_kernel(GroupList L, unsigned long long *__restrict__ ext) {
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  GroupCarry<unsigned long long> carry;
  carry.g = -1;
#pragma unroll 1
  for (int k = 0; k < kGsGatherRows; k++) {
    const int64_t row = ((int64_t)blockIdx.x * (kGsBlock / 64) + wave) * kGsGatherRows + k;
    int32_t g;
    float x, y, z;
    const bool live = gs_member(L, row * kGsRow + lane, g, x, y, z);
    if (__ballot(g >= 0) == 0ull) break;  // uniform: the list ended
    unsigned long long lo[3], hi[3];
    const unsigned long long kxy = hull_key(x, y), kyx = hull_key(y, x);
    lo[0] = lo[2] = live ? kxy : kGroupKeyMin64;
    lo[1] = live ? kyx : kGroupKeyMin64;
    hi[0] = hi[2] = live ? kxy : kGroupKeyMax64;
    hi[1] = live ? kyx : kGroupKeyMax64;
    // (all ones is a NaN's key twice: no live member's)
    gs_combine_row(g, lo, hi, lane, carry, ext, (unsigned long long)kGroupKeyMin64);
  }
  carry.flush(ext, lane, (unsigned long long)kGroupKeyMin64);
}

__device__ __forceinline__ int gh_orient(const uint64_t a, const uint64_t b, const uint64_t c) {
  return hull_orient(hull_key_x(a), hull_key_y(a), hull_key_x(b), hull_key_y(b), hull_key_x(c), hull_key_y(c));
}
__device__ __forceinline__ uint64_t gh_swap(const uint64_t k) { return (k << 32) | (k >> 32); }  // a (y, x) key as (x, y)

// ------------------------------------------------------------------ filter
// a lane per slot of the mapped tiles: xy[slot] = the place's key, gk[slot] = 2 group + class or kGhDead, kid[slot] = id
__global__ __launch_bounds__(kGsBlock) void gh_filter_kernel(GroupList L, const unsigned long long *__restrict__ ext,
                                                             uint64_t *__restrict__ xy, uint32_t *__restrict__ gk,
                                                             uint32_t *__restrict__ kid) {
  const int64_t slot = (int64_t)blockIdx.x * kGsBlock + threadIdx.x;
  int32_t g;
  float x, y, z;
  const bool live = gs_member(L, slot, g, x, y, z);
  uint64_t key = ~0ull;
  uint32_t cls = kGhDead, id = kGhDead;
  if (live) {
    key = hull_key(x, y);
    id = (uint32_t)L.ids[slot];
    const unsigned long long *e = ext + 6 * (size_t)g;
    const uint64_t kl = e[0], kr = e[3];
    if (key == kl || key == kr) {
      cls = 2u * (uint32_t)g;
    } else {
      const int side = gh_orient(kl, kr, key);
      if (side < 0) {
        const uint64_t kb = gh_swap(e[1]);
        if (!(gh_orient(kl, kb, key) > 0 && gh_orient(kb, kr, key) > 0)) cls = 2u * (uint32_t)g;
      } else if (side > 0) {
        const uint64_t kt = gh_swap(e[4]);
        if (!(gh_orient(kr, kt, key) > 0 && gh_orient(kt, kl, key) > 0)) cls = 2u * (uint32_t)g + 1u;
      }
    }
  }
  xy[slot] = key;
  gk[slot] = cls;
  kid[slot] = id;
}

// ------------------------------------------------------------------ sort keys
// key[i] of the entry vals[i] (a slot; vals == nullptr: i itself) for the next pass: 0 the id, 1 the y key, 2 the x key,
// 3 the (group, class) key
__global__ __launch_bounds__(256) void gh_key_kernel(int mode, const uint32_t *__restrict__ vals, int64_t n,
                                                     const uint64_t *__restrict__ xy, const uint32_t *__restrict__ gk,
                                                     const uint32_t *__restrict__ kid, uint32_t *__restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t s = vals ? (size_t)vals[i] : (size_t)i;
  key[i] = mode == 0 ? kid[s] : (mode == 1 ? (uint32_t)xy[s] : (mode == 2 ? (uint32_t)(xy[s] >> 32) : gk[s]));
}

// ------------------------------------------------------------------ compaction
// flag[i] = is sorted entry i the first of its (group, class, place)?; cnt[0] = n
__global__ __launch_bounds__(256) void gh_head_kernel(const uint32_t *__restrict__ sv, int64_t n,
                                                      const uint64_t *__restrict__ xy, const uint32_t *__restrict__ gk,
                                                      uint8_t *__restrict__ flag, uint32_t *__restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) cnt[0] = (uint32_t)n;
  if (i >= n) return;
  const uint32_t s = sv[i];
  bool head = gk[s] != kGhDead;
  if (head && i > 0) {
    const uint32_t p = sv[i - 1];
    head = gk[p] != gk[s] || xy[p] != xy[s];
  }
  flag[i] = head ? 1 : 0;
}

__global__ __launch_bounds__(256) void gh_flag_count_kernel(const uint8_t *__restrict__ flag, const uint32_t *__restrict__ d_n,
                                                            uint32_t *__restrict__ tile_count) {
  tile_flag_count((int64_t)*d_n, [&](int64_t j) { return flag[j] != 0; }, tile_count);
}
__global__ __launch_bounds__(1024) void gh_flag_scan_kernel(uint32_t *__restrict__ tile_count, int ntiles,
                                                            uint32_t *__restrict__ total) {
  tile_scan(tile_count, ntiles, total);
}
__global__ __launch_bounds__(256) void gh_flag_write_kernel(const uint8_t *__restrict__ flag, const uint32_t *__restrict__ d_n,
                                                            const uint32_t *__restrict__ tile_offset,
                                                            const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
  tile_flag_write((int64_t)*d_n, [&](int64_t j) { return flag[j] != 0; }, tile_offset,
                  [=](uint32_t at, int64_t j) { out[at] = in[j]; });
}

// ------------------------------------------------------------------ reduce
// does b stay on the chain of class `sgn` (+1 lower: left turns, -1 upper: right turns) between a and p?
__device__ __forceinline__ bool gh_stays(const uint64_t a, const uint64_t b, const uint64_t p, const int sgn) {
  return sgn * gh_orient(a, b, p) > 0;
}

// a lane per kGhChunk consecutive entries of list[0 .. *d_n): flag[i] = does entry i stay?
__global__ __launch_bounds__(256) void gh_reduce_kernel(const uint32_t *__restrict__ list, const uint32_t *__restrict__ d_n,
                                                        const uint64_t *__restrict__ xy, const uint32_t *__restrict__ gk,
                                                        const unsigned long long *__restrict__ ext,
                                                        uint8_t *__restrict__ flag) {
  __shared__ uint64_t s_key[kGhChunk * 256];  // the lane's stack, lane-major: no two lanes share a bank's word
  __shared__ uint8_t s_ix[kGhChunk * 256];
  const int64_t n = (int64_t)*d_n;
  const int64_t base = ((int64_t)blockIdx.x * 256 + threadIdx.x) * kGhChunk;
  if (base >= n) return;
  uint32_t keep = 0u, cur = kGhDead;
  int top = 0, sgn = 1;
  uint64_t kl = 0ull, kr = 0ull;
  const int t = (int)threadIdx.x;
#define GH_POP_WHILE_OFF(P)                                                                        \
  while (top >= 1) {                                                                               \
    const uint64_t b = s_key[(top - 1) * 256 + t], a = top >= 2 ? s_key[(top - 2) * 256 + t] : kl; \
    if (gh_stays(a, b, (P), sgn)) break;                                                           \
    keep &= ~(1u << s_ix[(top - 1) * 256 + t]);                                                    \
    top--;                                                                                         \
  }
#pragma unroll 1
  for (int j = 0; j < kGhChunk && base + j < n; j++) {
    const uint32_t s = list[base + j];
    const uint32_t k = gk[s];
    const uint64_t key = xy[s];
    if (k != cur) {  // the next (group, class): close the chain of the last one at R
      if (cur != kGhDead) GH_POP_WHILE_OFF(kr)
      cur = k;
      top = 0;
      sgn = (k & 1u) ? -1 : 1;
      kl = ext[6 * (size_t)(k >> 1)];
      kr = ext[6 * (size_t)(k >> 1) + 3];
    }
    keep |= 1u << j;
    if (key == kl || key == kr) continue;  // the anchors themselves stay and stand on no stack
    GH_POP_WHILE_OFF(key)
    s_key[top * 256 + t] = key;
    s_ix[top * 256 + t] = (uint8_t)j;
    top++;
  }
  if (cur != kGhDead) GH_POP_WHILE_OFF(kr)
#undef GH_POP_WHILE_OFF
  uint4 out;
  uint32_t *o4 = reinterpret_cast<uint32_t *>(&out);
#pragma unroll
  for (int w = 0; w < 4; w++)
    o4[w] = ((keep >> (4 * w)) & 1u) | (((keep >> (4 * w + 1)) & 1u) << 8) | (((keep >> (4 * w + 2)) & 1u) << 16) |
            (((keep >> (4 * w + 3)) & 1u) << 24);
  *reinterpret_cast<uint4 *>(flag + base) = out;  // (flag holds whole chunks)
}
static_assert(kGhChunk == 16, "a lane's keep flags are one 16-byte store");

// ------------------------------------------------------------------ chain
// seg_lo / seg_hi[k] = the stretch of (group, class) k in list[0 .. *d_n); zero where it has none (set before)
__global__ __launch_bounds__(256) void gh_bounds_kernel(const uint32_t *__restrict__ list, const uint32_t *__restrict__ d_n,
                                                        const uint32_t *__restrict__ gk, uint32_t *__restrict__ seg_lo,
                                                        uint32_t *__restrict__ seg_hi) {
  const int64_t n = (int64_t)*d_n;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = gk[list[i]];
  if (i == 0 || gk[list[i - 1]] != k) seg_lo[k] = (uint32_t)i;
  if (i == n - 1 || gk[list[i + 1]] != k) seg_hi[k] = (uint32_t)(i + 1);
}

// a lane per group: the chains of its two classes over what is left, the stack of class c in stk[seg_lo .. ); n_low[g]:
// the vertices of the lower chain (L and R with it), hs[g]: all of them
__global__ __launch_bounds__(256) void gh_chain_kernel(int32_t cap_groups, const uint32_t *__restrict__ list,
                                                       const uint64_t *__restrict__ xy,
                                                       const unsigned long long *__restrict__ ext,
                                                       const uint32_t *__restrict__ seg_lo, const uint32_t *__restrict__ seg_hi,
                                                       uint32_t *__restrict__ stk, int32_t *__restrict__ n_low,
                                                       int32_t *__restrict__ hs, int32_t *__restrict__ hull_sizes) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)cap_groups) return;
  int32_t count[2] = {0, 0};
#pragma unroll 1
  for (int c = 0; c < 2; c++) {
    const uint32_t lo = seg_lo[2 * g + c], hi = seg_hi[2 * g + c];
    if (hi <= lo) continue;  // (a group without this class; a group without a live member has no keys either)
    const uint64_t kl = ext[6 * (size_t)g], kr = ext[6 * (size_t)g + 3];
    const int sgn = c ? -1 : 1;
    uint32_t *st = stk + lo;
    int64_t pre = 0, top = 0;
    uint32_t last = kGhDead;
    for (uint32_t i = lo; i < hi; i++) {
      const uint32_t s = list[i];
      const uint64_t key = xy[s];
      if (key == kl) {  // (the first entry of class 0)
        st[0] = s;
        pre = 1;
        continue;
      }
      if (key == kr) {  // (the last entry of class 0)
        last = s;
        continue;
      }
      while (top >= 1) {
        const uint64_t b = xy[st[pre + top - 1]], a = top >= 2 ? xy[st[pre + top - 2]] : kl;
        if (gh_stays(a, b, key, sgn)) break;
        top--;
      }
      st[pre + top] = s;
      top++;
    }
    while (top >= 1) {
      const uint64_t b = xy[st[pre + top - 1]], a = top >= 2 ? xy[st[pre + top - 2]] : kl;
      if (gh_stays(a, b, kr, sgn)) break;
      top--;
    }
    if (last != kGhDead) {
      st[pre + top] = last;
      top++;
    }
    count[c] = (int32_t)(pre + top);
  }
  n_low[g] = count[0];
  hs[g] = count[0] + count[1];
  if (hull_sizes) hull_sizes[g] = count[0] + count[1];
}

// ------------------------------------------------------------------ finish
// a lane per group: hv[H_g ..] = the slots of its vertices, counter-clockwise from L; hull_ids[H_g ..] = their ids
__global__ __launch_bounds__(256) void gh_write_kernel(int32_t cap_groups, const int32_t *__restrict__ hs,
                                                       const int32_t *__restrict__ n_low, const int32_t *__restrict__ hoff,
                                                       const uint32_t *__restrict__ seg_lo, const uint32_t *__restrict__ stk,
                                                       const uint32_t *__restrict__ kid, uint32_t *__restrict__ hv,
                                                       int32_t *__restrict__ hull_ids) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)cap_groups) return;
  const int32_t h = hs[g], n0 = n_low[g];
  const int64_t H = (int64_t)hoff[g];
  const uint32_t *low = stk + seg_lo[2 * g], *up = stk + seg_lo[2 * g + 1];
  for (int32_t k = 0; k < h; k++) {
    const uint32_t s = k < n0 ? low[k] : up[h - 1 - k];  // (the upper chain backwards: its entry h - n0 - 1 - (k - n0))
    hv[H + k] = s;
    if (hull_ids) hull_ids[H + k] = (int32_t)kid[s];
  }
}

// The fan's shoelace terms of the hull v[0 .. h) added in order, halved
__device__ __forceinline__ double gh_area(const uint32_t *__restrict__ v, const uint64_t *__restrict__ xy, const int32_t h) {
  if (h < 3) return 0.0;
  const uint64_t k0 = xy[v[0]];
  uint64_t kb = xy[v[1]];
  double a = 0.0;
  for (int32_t k = 1; k + 1 < h; k++) {
    const uint64_t ka = kb;
    kb = xy[v[k + 1]];
    a += hull_shoelace(hull_key_x(k0), hull_key_y(k0), hull_key_x(ka), hull_key_y(ka), hull_key_x(kb), hull_key_y(kb));
  }
  return a * 0.5;
}

// The extents of all h vertices about edge k (h >= 2)
__device__ __forceinline__ HullExtents gh_edge(const uint32_t *__restrict__ v, const uint64_t *__restrict__ xy, const int32_t h,
                                               const int32_t k) {
  const uint64_t ka = xy[v[k]], kb = xy[v[k + 1 < h ? k + 1 : 0]];
  HullExtents E;
  E.start(hull_key_x(ka), hull_key_y(ka), hull_key_x(kb), hull_key_y(kb));
  for (int32_t j = 0; j < h; j++) {
    const uint64_t kp = xy[v[j]];
    E.add(hull_key_x(kp), hull_key_y(kp));
  }
  if (h == 2) E.lo_n = E.hi_n = 0.0;  // a segment has no width
  return E;
}

// The smallest product among the edges first, first + step, ... (ascending: a strict comparison keeps the first)
__device__ __forceinline__ void gh_best_edge(const uint32_t *__restrict__ v, const uint64_t *__restrict__ xy, const int32_t h,
                                             const int32_t first, const int32_t step, double &best, int32_t &best_k) {
  const int32_t edges = h == 2 ? 1 : h;
  best = 0.0;
  best_k = -1;
  for (int32_t k = first; k < edges; k += step) {
    const double a = gh_edge(v, xy, h, k).area();
    if (best_k < 0 || a < best) {
      best = a;
      best_k = k;
    }
  }
}

constexpr int kGhLaneHull = 16;  // a hull of up to this many vertices is finished by its own lane

// a lane per row g of [0, cap_groups): area[g] and rect[6 g ..] of a hull of up to kGhLaneHull vertices; a longer one by
// the whole wave (a lane per edge, h^2 work with shared loads), as gs_frame_kernel sums a long group.  The products are
// the same expressions either way, and of equal ones the first edge wins either way.
__global__ __launch_bounds__(256) void gh_rect_kernel(int32_t cap_groups, const int32_t *__restrict__ hs,
                                                      const int32_t *__restrict__ hoff, const uint32_t *__restrict__ hv,
                                                      const uint64_t *__restrict__ xy, double *__restrict__ area,
                                                      double *__restrict__ rect) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = g < (int64_t)cap_groups;
  const int32_t h = in ? hs[g] : 0, at = in ? hoff[g] : 0;
  const uint32_t *v = hv + at;
  double a = 0.0, out[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (h == 1) {
    const uint64_t k0 = xy[v[0]];
    out[0] = (double)hull_key_x(k0);
    out[1] = (double)hull_key_y(k0);
    out[2] = 1.0;
  } else if (h >= 2 && h <= kGhLaneHull) {
    if (area) a = gh_area(v, xy, h);
    if (rect) {
      double best;
      int32_t best_k;
      gh_best_edge(v, xy, h, 0, 1, best, best_k);
      gh_edge(v, xy, h, best_k).rect(out);
    }
  }
  unsigned long long todo = __ballot(h > kGhLaneHull);
  while (todo) {  // uniform: the wave finishes one long hull
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t lh = __shfl(h, leader);
    const uint32_t *lv = hv + __shfl(at, leader);
    if (area) {
      const double la = gh_area(lv, xy, lh);  // (every lane the same terms in the same order)
      if (lane == leader) a = la;
    }
    if (rect) {
      double best;
      int32_t best_k;
      gh_best_edge(lv, xy, lh, lane, 64, best, best_k);
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {  // the smallest product, of equal ones the first edge
        const double oa = __shfl_xor(best, m);
        const int32_t ok = __shfl_xor(best_k, m);
        if (ok >= 0 && (best_k < 0 || oa < best || (oa == best && ok < best_k))) {
          best = oa;
          best_k = ok;
        }
      }
      double lo[6];
      gh_edge(lv, xy, lh, best_k).rect(lo);
      if (lane == leader)
#pragma unroll
        for (int k = 0; k < 6; k++) out[k] = lo[k];
    }
    todo &= todo - 1ull;
  }
  if (!in) return;
  if (area) area[g] = a;
  if (rect)
#pragma unroll
    for (int k = 0; k < 6; k++) rect[6 * (size_t)g + k] = out[k];
}

// ------------------------------------------------------------------ the call
struct HullOut {
  int32_t *hull_sizes;  // [cap_groups]
  int32_t *hull_ids;    // [cap_ids]
  double *area;         // [cap_groups]
  double *rect;         // [6 cap_groups]
};

static pcgx_status gh_empty_outputs(const HullOut &O, int64_t cap_ids, int64_t cap_groups, hipStream_t st) {
  if (O.hull_sizes) PCGX_HIP_TRY(hipMemsetAsync(O.hull_sizes, 0, (size_t)cap_groups * 4, st));
  if (O.hull_ids && cap_ids > 0) PCGX_HIP_TRY(hipMemsetAsync(O.hull_ids, 0xff, (size_t)cap_ids * 4, st));
  if (O.area) PCGX_HIP_TRY(hipMemsetAsync(O.area, 0, (size_t)cap_groups * 8, st));
  if (O.rect) PCGX_HIP_TRY(hipMemsetAsync(O.rect, 0, (size_t)cap_groups * 48, st));
  return PCGX_OK;
}

static int gh_bits_for(uint64_t top) {  // bits that hold every value of [0, top]
  int b = 1;
  while (b < 32 && (top >> b) != 0) b++;
  return b;
}

// Len() > 0, cap_ids > 0, cap_groups > 0, everything device resident; temporaries from ctx().arena
static pcgx_status group_hulls_enqueue(const pcgx_kdtree *t, const int32_t *d_ids, int64_t cap_ids, const int32_t *d_sizes,
                                       int64_t cap_groups, const int32_t *d_n_groups, const HullOut &O, hipStream_t st) {
  Arena &ar = ctx().arena;
  PCGX_TRY(ar.begin(st));
  const uint32_t *inv = nullptr;
  PCGX_TRY(range_inverse_map(t, &inv, st));
  const int64_t entries = cap_groups + 1;
  const unsigned scan_tiles = (unsigned)((entries + kGsTile - 1) / kGsTile);
  const unsigned gather_tiles = (unsigned)((cap_ids + kGsGatherTile - 1) / kGsGatherTile);
  const unsigned slot_tiles = gather_tiles * (kGsGatherTile / kGsTile);
  const size_t slots = (size_t)slot_tiles * kGsTile;  // (>= cap_ids)
  const unsigned group_blocks = (unsigned)((cap_groups + 255) / 256);
  const unsigned id_blocks = (unsigned)((cap_ids + 255) / 256);
  const int run_tiles = (int)((cap_ids + kRunTile - 1) / kRunTile);
  const int64_t chunks = (cap_ids + kGhChunk - 1) / kGhChunk;
  const unsigned chunk_blocks = (unsigned)((chunks + 255) / 256);
  uint64_t *tile_sum = nullptr, *xy = nullptr;
  int32_t *off = nullptr, *grp = nullptr, *hs = nullptr, *n_low = nullptr, *hoff = nullptr;
  unsigned long long *ext = nullptr;
  uint32_t *gk = nullptr, *kid = nullptr, *keys[2] = {nullptr, nullptr}, *vals[2] = {nullptr, nullptr};
  uint32_t *list[2] = {nullptr, nullptr}, *stk = nullptr, *seg = nullptr, *hv = nullptr, *tile_count = nullptr, *cnt = nullptr;
  uint8_t *flag = nullptr;
  void *ws = nullptr;
  PCGX_TRY(ar.alloc_n((size_t)scan_tiles, &tile_sum));
  PCGX_TRY(ar.alloc_n((size_t)entries, &off));
  PCGX_TRY(ar.alloc_n(slots + 4, &grp));
  PCGX_TRY(ar.alloc_n((size_t)cap_groups * 6, &ext));
  PCGX_TRY(ar.alloc_n(slots, &xy));
  PCGX_TRY(ar.alloc_n(slots, &gk));
  PCGX_TRY(ar.alloc_n(slots, &kid));
  for (int k = 0; k < 2; k++) {
    PCGX_TRY(ar.alloc_n((size_t)cap_ids, &keys[k]));
    PCGX_TRY(ar.alloc_n((size_t)cap_ids, &vals[k]));
    PCGX_TRY(ar.alloc_n((size_t)cap_ids, &list[k]));
  }
  PCGX_TRY(ar.alloc(radix_sort_workspace_bytes(cap_ids), &ws));
  PCGX_TRY(ar.alloc_n((size_t)chunks * kGhChunk, &flag));
  PCGX_TRY(ar.alloc_n((size_t)run_tiles + 1, &tile_count));
  PCGX_TRY(ar.alloc_n((size_t)kGhRounds + 2, &cnt));
  PCGX_TRY(ar.alloc_n((size_t)cap_ids, &stk));
  PCGX_TRY(ar.alloc_n((size_t)cap_groups * 4, &seg));
  PCGX_TRY(ar.alloc_n((size_t)cap_groups, &hs));
  PCGX_TRY(ar.alloc_n((size_t)cap_groups, &n_low));
  PCGX_TRY(ar.alloc_n((size_t)entries, &hoff));
  PCGX_TRY(ar.alloc_n((size_t)cap_ids, &hv));
  const int32_t cg = (int32_t)cap_groups, ci = (int32_t)cap_ids;
  // offsets, map, extremes, filter
  group_scan_launch(d_sizes, d_n_groups, cg, ci, tile_sum, scan_tiles, st);
  hipLaunchKernelGGL(gh_offsets_kernel<true>, dim3(scan_tiles), dim3(kGsBlock), 0, st, d_sizes, d_n_groups, cg, ci,
                     (const uint64_t *)tile_sum, off, ext);
  group_map_launch(off, d_n_groups, cg, grp, slot_tiles, st);
  const GroupList L{t->d_nodes, inv, t->n, d_ids, grp};
  hipLaunchKernelGGL(gh_extreme_kernel, dim3(gather_tiles), dim3(kGsBlock), 0, st, L, ext);
  hipLaunchKernelGGL(gh_filter_kernel, dim3((unsigned)(slots / kGsBlock)), dim3(kGsBlock), 0, st, L,
                     (const unsigned long long *)ext, xy, gk, kid);
  PCGX_HIP_TRY(hipGetLastError());
  // sort: id, y, x, (group, class); each pass's keys are gathered through the last pass's order
  const int bits[4] = {gh_bits_for((uint64_t)t->n - 1), 32, 32, gh_bits_for(2 * (uint64_t)cap_groups)};
  for (int pass = 0; pass < 4; pass++) {
    hipLaunchKernelGGL(gh_key_kernel, dim3(id_blocks), dim3(256), 0, st, pass, pass ? (const uint32_t *)vals[0] : nullptr,
                       cap_ids, (const uint64_t *)xy, (const uint32_t *)gk, (const uint32_t *)kid, keys[0]);
    int r = 0;
    PCGX_TRY(radix_sort_pairs(keys, vals, cap_ids, bits[pass], ws, &r, st, pass == 0));
    if (r) {  // the next pass reads, and the heads read, buffer 0
      uint32_t *a = keys[0], *b = vals[0];
      keys[0] = keys[1], keys[1] = a;
      vals[0] = vals[1], vals[1] = b;
    }
  }
  const uint32_t *sv = vals[0];
  // heads, then the reduce rounds: list r -> flags -> list r + 1
  hipLaunchKernelGGL(gh_head_kernel, dim3(id_blocks), dim3(256), 0, st, sv, cap_ids, (const uint64_t *)xy, (const uint32_t *)gk,
                     flag, cnt);
  const uint32_t *in = sv;
  for (int r = 0; r <= kGhRounds; r++) {
    uint32_t *out = list[r & 1];
    hipLaunchKernelGGL(gh_flag_count_kernel, dim3(run_tiles), dim3(256), 0, st, (const uint8_t *)flag, (const uint32_t *)(cnt + r),
                       tile_count);
    hipLaunchKernelGGL(gh_flag_scan_kernel, dim3(1), dim3(1024), 0, st, tile_count, run_tiles, cnt + r + 1);
    hipLaunchKernelGGL(gh_flag_write_kernel, dim3(run_tiles), dim3(256), 0, st, (const uint8_t *)flag,
                       (const uint32_t *)(cnt + r), (const uint32_t *)tile_count, in, out);
    in = out;
    if (r < kGhRounds)
      hipLaunchKernelGGL(gh_reduce_kernel, dim3(chunk_blocks), dim3(256), 0, st, in, (const uint32_t *)(cnt + r + 1),
                         (const uint64_t *)xy, (const uint32_t *)gk, (const unsigned long long *)ext, flag);
  }
  PCGX_HIP_TRY(hipGetLastError());
  const uint32_t *d_left = cnt + kGhRounds + 1;
  // chain, the hull offsets, the vertices, area and rectangle
  uint32_t *seg_lo = seg, *seg_hi = seg + 2 * (size_t)cap_groups;
  PCGX_HIP_TRY(hipMemsetAsync(seg, 0, (size_t)cap_groups * 16, st));
  hipLaunchKernelGGL(gh_bounds_kernel, dim3(id_blocks), dim3(256), 0, st, in, d_left, (const uint32_t *)gk, seg_lo, seg_hi);
  hipLaunchKernelGGL(gh_chain_kernel, dim3(group_blocks), dim3(256), 0, st, cg, in, (const uint64_t *)xy,
                     (const unsigned long long *)ext, (const uint32_t *)seg_lo, (const uint32_t *)seg_hi, stk, n_low, hs,
                     O.hull_sizes);
  group_scan_launch(hs, nullptr, cg, ci, tile_sum, scan_tiles, st);
  hipLaunchKernelGGL(gh_offsets_kernel<false>, dim3(scan_tiles), dim3(kGsBlock), 0, st, (const int32_t *)hs,
                     (const int32_t *)nullptr, cg, ci, (const uint64_t *)tile_sum, hoff, (unsigned long long *)nullptr);
  if (O.hull_ids) PCGX_HIP_TRY(hipMemsetAsync(O.hull_ids, 0xff, (size_t)cap_ids * 4, st));
  hipLaunchKernelGGL(gh_write_kernel, dim3(group_blocks), dim3(256), 0, st, cg, (const int32_t *)hs, (const int32_t *)n_low,
                     (const int32_t *)hoff, (const uint32_t *)seg_lo, (const uint32_t *)stk, (const uint32_t *)kid, hv,
                     O.hull_ids);
  if (O.area || O.rect)
    hipLaunchKernelGGL(gh_rect_kernel, dim3(group_blocks), dim3(256), 0, st, cg, (const int32_t *)hs,
                       (const int32_t *)hoff, (const uint32_t *)hv, (const uint64_t *)xy, O.area, O.rect);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kHullMax = 0x7fffffff;  // slots, groups and ids are int32 on the device

pcgx_status group_hulls_check(const char *fn, const pcgx_kdtree *t, const void *ids, int64_t n_ids, const void *sizes,
                              int64_t n_groups) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (n_ids < 0 || n_groups < 0) return fail(PCGX_E_INVALID, "%s: negative number of ids or groups", fn);
  if (n_ids > kHullMax || n_groups > kHullMax || t->n > kHullMax)
    return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 slots, groups or points", fn);
  if (n_ids > 0 && !ids) return fail(PCGX_E_INVALID, "%s: NULL ids", fn);
  if (n_groups > 0 && !sizes) return fail(PCGX_E_INVALID, "%s: NULL sizes", fn);
  return PCGX_OK;
}

}  // namespace

extern "C" int32_t pcgx_group_hulls_chunk(void) { return kGhChunk; }

extern "C" pcgx_status pcgx_kdtree_group_hulls_dev(const pcgx_kdtree *t, const int32_t *d_ids, int64_t cap_ids,
                                                   const int32_t *d_sizes, int64_t cap_groups, const int32_t *d_n_groups,
                                                   int32_t *d_hull_sizes, int32_t *d_hull_ids, double *d_area,
                                                   double *d_rect, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(group_hulls_check("pcgx_kdtree_group_hulls_dev", t, d_ids, cap_ids, d_sizes, cap_groups));
  if (cap_groups == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  const HullOut O{d_hull_sizes, d_hull_ids, d_area, d_rect};
  if (t->n == 0 || cap_ids == 0) return gh_empty_outputs(O, cap_ids, cap_groups, st);  // no point, no slot: nothing is live
  return group_hulls_enqueue(t, d_ids, cap_ids, d_sizes, cap_groups, d_n_groups, O, st);
}

extern "C" pcgx_status pcgx_kdtree_group_hulls(const pcgx_kdtree *t, const int64_t *ids, int64_t n_ids, const int64_t *sizes,
                                               int64_t n_groups, int64_t *hull_sizes, int64_t *hull_ids, double *area,
                                               double *rect) {
  PCGX_API_CALL();
  PCGX_TRY(group_hulls_check("pcgx_kdtree_group_hulls", t, ids, n_ids, sizes, n_groups));
  if (n_groups == 0) return PCGX_OK;
  const int64_t n = t->n;
  RawVector<int32_t> h((size_t)n_ids + (size_t)n_groups);  // the ids, then the sizes
  for (int64_t s = 0; s < n_ids; s++) {
    if (ids[s] < 0 || ids[s] >= n) return fail(PCGX_E_INVALID, "pcgx_kdtree_group_hulls: id out of range");
    h[(size_t)s] = (int32_t)ids[s];
  }
  int64_t sum = 0;
  for (int64_t g = 0; g < n_groups; g++) {
    const int64_t s = sizes[g] < 0 ? 0 : sizes[g];
    if (s > n_ids - sum) return fail(PCGX_E_INVALID, "pcgx_kdtree_group_hulls: the sizes add up to more than n_ids");
    sum += s;
    h[(size_t)(n_ids + g)] = (int32_t)s;
  }
  PCGX_TRY(ensure_init());
  // always on the device: the hulls are the kernels', not a host restatement
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  const size_t G = (size_t)n_groups, S = (size_t)n_ids;
  int32_t *d_in = nullptr, *d_hs = nullptr, *d_hi = nullptr;
  double *d_area = nullptr, *d_rect = nullptr;
  PCGX_TRY(ha.alloc_n(h.size(), &d_in));
  PCGX_TRY(staged_upload(d_in, h.data(), h.size() * 4, st));
  if (hull_sizes) PCGX_TRY(ha.alloc_n(G, &d_hs));
  if (hull_ids && S) PCGX_TRY(ha.alloc_n(S, &d_hi));
  if (area) PCGX_TRY(ha.alloc_n(G, &d_area));
  if (rect) PCGX_TRY(ha.alloc_n(G * 6, &d_rect));
  PCGX_TRY(pcgx_kdtree_group_hulls_dev(t, d_in, n_ids, d_in + n_ids, n_groups, nullptr, d_hs, d_hi, d_area, d_rect, st));
  if (hull_sizes) {
    RawVector<int32_t> c(G);
    PCGX_TRY(staged_download(c.data(), d_hs, G * 4, st));
    for (size_t g = 0; g < G; g++) hull_sizes[g] = c[g];
  }
  if (hull_ids && S) {
    RawVector<int32_t> c(S);
    PCGX_TRY(staged_download(c.data(), d_hi, S * 4, st));
    for (size_t s = 0; s < S; s++) hull_ids[s] = c[s];
  }
  if (area) PCGX_TRY(staged_download(area, d_area, G * 8, st));
  if (rect) PCGX_TRY(staged_download(rect, d_rect, G * 48, st));
  return PCGX_OK;
}
