// orient.hip -- consistent normal orientation over a tree's own points: the sign parity along the minimum spanning
// forest of the radius graph, by Boruvka rounds (extension: no reference parity; include/pcgx.h, "consistent normal
// orientation"; the rules are orient_terms.h's).
//
// State by point id: one packed node word {parent, parity} (orient_terms.h states the invariant), flattened at the end of
// every round, so that in a round node[j] >> 1 IS j's root; a byte "usable"; per root two 64-bit choice words.
// A round:
//   orient_edge_kernel    one more consumer of the shared enumeration (radius_visit.h), one still-active point per lane:
//                         it keeps in registers the first edge, by the edge order, to a usable neighbour under a DIFFERENT
//                         root, and the wave puts the largest weight per distinct root into best_w[root] (atomicMax).
//                         The node words are only read here.  A point with no such neighbour can never offer an edge
//                         again (components only grow) and leaves the active list.
//   orient_tie_kernel     the lanes whose weight IS their root's maximum put their pair word into best_p[root]
//                         (atomicMin): the component's first leaving edge, whichever lanes ran when.
//   orient_count / scan / write kernels   the still-active records, in order, into the other list buffer.
//   orient_offer_kernel   only on a handle that holds a NaN coordinate, where neighbourhoods need not be symmetric.
//   orient_hook_kernel    one lane per root with a choice (a, b): mutual choices are one edge, and the larger root hooks
//                         under the smaller; else the root hooks under whatever b's word names.
//   orient_jump_kernel    parity pointer jumping until every word names a root; puts the choice words back to "none".
// Why a hook may read words other lanes are writing: only roots' words are written, each once, by its own lane.  a's
// word is a non-root's (stable) or the lane's own.  b's word is stable, or B's own before or after B hooked: either way
// an ancestor of b with b's parity relative to it.  The chosen edges form no cycle but the mutual pair (a cycle
// A -> B -> ... -> A of first leaving edges would have to descend strictly in the edge order all the way round), so b's
// word names A only when B chose the same edge and has hooked already: then A must not.
// After the rounds: one more orient_edge_kernel marks the roots that still have a leaving edge (n_open); roots -> the
// smallest member id (wave_root_flush); the anchor or the votes per component; a sign per component; the outputs.
// Every round's kernels read the active count from a device word and return at once when it is zero; nothing waits on
// another workgroup; nothing is read back by the device form.
#include <math.h>
#include <stdlib.h>

#include "bucket_grid.h"
#include "orient_terms.h"
#include "radius_graph.h"
#include "radius_visit.h"

#ifndef PCGX_ORIENT_ACTIVE_LIST
#define PCGX_ORIENT_ACTIVE_LIST 1  // 0: every point stays in the list (measurements: what the list buys)
#endif

namespace pcgx {

constexpr int kOrientBlock = kRangeWalkBlock;  // one wave per workgroup: the walks' LDS frame stacks are [level][64]
constexpr bool kOrientActiveList = PCGX_ORIENT_ACTIVE_LIST != 0;

__device__ __forceinline__ uint32_t node_load(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ void node_store(uint32_t *p, const uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

__device__ __forceinline__ uint64_t shfl_xor_u64(const uint64_t v, const int o) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
  return ((uint64_t)hi << 32) | lo;
}

// One 64-bit word per lane -> words[root], combined per distinct root of the wave first (same-address atomics are
// served one after the other: wave_root_flush's reason).  All 64 lanes call it.  kOp: 0 atomicMax, 1 atomicMin, 2 atomicAdd.
template <int kOp>
__device__ __forceinline__ void wave_root_combine(const bool valid, const uint32_t root, const uint64_t word, const int lane,
                                                  unsigned long long *__restrict__ words) {
  unsigned long long todo = __ballot(valid);
  const uint64_t neutral = kOp == 1 ? ~0ull : 0ull;
  while (todo) {  // uniform
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)root, leader);
    const bool mine = valid && root == r;
    const unsigned long long same = __ballot(mine);
    uint64_t m = mine ? word : neutral;
    if (same & (same - 1ull)) {  // more than one lane under this root
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const uint64_t v = shfl_xor_u64(m, o);
        if (kOp == 0) m = v > m ? v : m;
        else if (kOp == 1) m = v < m ? v : m;
        else m += v;
      }
    }
    if (lane == leader) {
      if (kOp == 0) {
        if (m > __atomic_load_n(words + r, __ATOMIC_RELAXED)) atomicMax(words + r, (unsigned long long)m);
      } else if (kOp == 1) {
        if (m < __atomic_load_n(words + r, __ATOMIC_RELAXED)) atomicMin(words + r, (unsigned long long)m);
      } else if (m != 0ull) {
        atomicAdd(words + r, (unsigned long long)m);
      }
    }
    todo &= ~same;
  }
}

// What the kernels share: by id unless said otherwise.
struct OrientState {
  const float *normals;        // [3 n], as given
  uint32_t *node;              // the packed words
  uint8_t *ok;                 // usable (known from round 1 on)
  unsigned long long *best_w;  // per root: the largest weight key offered this round, 0 none
  unsigned long long *best_p;  // per root: the smallest pair word among the offers of that weight
  unsigned long long *in_w;    // per root, handles with a NaN coordinate only: the same two words over the choices of
  unsigned long long *in_p;    // OTHER roots that point at this one (nullptr elsewhere)
  uint64_t *lane_w, *lane_p;   // by list position: the lane's own first edge
  uint8_t *keep;               // by list position: stays in the active list
  uint32_t *min_id;            // per root: the component's smallest member id
  unsigned long long *sig;     // per root: mode 1 the anchor key, mode 2 the votes
  uint8_t *sigma;              // per root: the component's sign
  uint32_t *totals;            // {components, open components}
};

__global__ __launch_bounds__(256) void orient_prep_kernel(QuerySource Q, OrientState S, float4 *__restrict__ list,
                                                          uint32_t *__restrict__ count) {
  const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pos == 0) {
    *count = (uint32_t)Q.nq;
    S.totals[0] = 0u;
    S.totals[1] = 0u;
  }
  if (pos >= Q.nq) return;
  int64_t i = 0;
  float qx, qy, qz;
  read_query(Q, pos, i, qx, qy, qz);
  list[pos] = make_float4(qx, qy, qz, __uint_as_float((uint32_t)i));
  S.node[i] = orient_node((uint32_t)i, 0u);
  S.ok[i] = 0;
  S.best_w[i] = 0ull;
  S.best_p[i] = kOrientNoPair;
  S.min_id[i] = 0xffffffffu;
  S.sig[i] = 0ull;
  if (S.in_w) {
    S.in_w[i] = 0ull;
    S.in_p[i] = kOrientNoPair;
  }
}

// one lane's first leaving edge
struct OrientBest {
  OrientEdge e;
  bool met;

  __device__ __forceinline__ void take(const OrientState &S, const float4 &p, const uint32_t i, const bool normal_ok,
                                       const uint32_t root, const float nx, const float ny, const float nz) {
    const uint32_t j = __float_as_uint(p.w);
    if (j == i) {
      met = true;
      return;
    }
    if (!normal_ok) return;
    if (orient_parent(S.node[j]) == root) return;
    const float mx = S.normals[3 * (size_t)j], my = S.normals[3 * (size_t)j + 1], mz = S.normals[3 * (size_t)j + 2];
    // (j is in somebody's neighbourhood: it is live and finite, so it is in its own -- except in a tree a NaN has put
    // out of order, where a pass before the rounds has found out who is)
    if (!orient_usable(S.in_w == nullptr || S.ok[j] != 0, mx, my, mz)) return;
    const OrientEdge f{orient_weight_key(orient_c(nx, ny, nz, mx, my, mz)), orient_pair(i, j)};
    if (orient_before(f, e)) e = f;
  }
  __device__ __forceinline__ void merge(const OrientEdge &f) {
    if (orient_before(f, e)) e = f;
  }
};

template <int kSrc>
__global__ __launch_bounds__(kOrientBlock) void orient_edge_kernel(GridView g, TreeView tv, XTreeView xv,
                                                                   const float4 *__restrict__ list,
                                                                   const uint32_t *__restrict__ count, float bound,
                                                                   OrientState S, int64_t guard) {
  extern __shared__ uint32_t s_stack[];
  const uint32_t cnt = *count;
  if (cnt == 0u) return;
  const uint32_t n_tiles = (cnt + kOrientBlock - 1) / kOrientBlock;
  if ((blockIdx.x >> 3) >= (n_tiles + 7u) / 8u) return;  // (xcd_tile beyond an XCD's share would name another's tile)
  const uint32_t tile = xcd_tile(blockIdx.x, n_tiles);
  if (tile >= n_tiles) return;
  const uint32_t pos = tile * kOrientBlock + threadIdx.x;
  const bool live = pos < cnt;
  uint32_t i = 0u, root = 0u;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
  bool normal_ok = false;
  if (live) {
    const float4 r = list[pos];
    i = __float_as_uint(r.w);
    qx = r.x; qy = r.y; qz = r.z;
    nx = S.normals[3 * (size_t)i]; ny = S.normals[3 * (size_t)i + 1]; nz = S.normals[3 * (size_t)i + 2];
    normal_ok = cluster_normal_ok(nx, ny, nz);
    root = orient_parent(S.node[i]);
  }
  OrientBest b{OrientEdge{0ull, kOrientNoPair}, false};
  const int lane = (int)(threadIdx.x & 63u);
  radius_visit<kSrc>(
      RadiusViews{g, tv, xv, guard}, s_stack + threadIdx.x, kOrientBlock, qx, qy, qz, bound, live && normal_ok,
      [&](const float4 &p, float) { b.take(S, p, i, normal_ok, root, nx, ny, nz); },
      [&](int owner, float, float, float, auto rows) {  // the wave's first edge of the owner's row, by shuffles
        const uint32_t oi = __shfl(i, owner), oroot = __shfl(root, owner);
        const float onx = __shfl(nx, owner), ony = __shfl(ny, owner), onz = __shfl(nz, owner);
        OrientBest part{OrientEdge{0ull, kOrientNoPair}, false};
        rows([&](const float4 &p, float) { part.take(S, p, oi, true, oroot, onx, ony, onz); });
        for (int o = 32; o > 0; o >>= 1)
          part.merge(OrientEdge{shfl_xor_u64(part.e.weight, o), shfl_xor_u64(part.e.pair, o)});
        const bool any_met = __ballot(part.met) != 0ull;
        if (lane == owner) {
          b.merge(part.e);
          b.met = b.met || any_met;
        }
      });
  // (no lane has left: the wave combines its offers per root)
  const bool usable = live && orient_usable(b.met, nx, ny, nz);
  const bool has = usable && b.e.weight != 0ull;
  wave_root_combine<0>(has, root, b.e.weight, lane, S.best_w);
  if (!live) return;
  if (usable) S.ok[i] = 1;
  S.lane_w[pos] = has ? b.e.weight : 0ull;
  S.lane_p[pos] = b.e.pair;
  S.keep[pos] = kOrientActiveList ? (has ? 1 : 0) : 1;
}

__global__ __launch_bounds__(256) void orient_tie_kernel(const float4 *__restrict__ list, const uint32_t *__restrict__ count,
                                                         OrientState S) {
  const uint32_t cnt = *count;
  if ((uint64_t)blockIdx.x * 256 >= cnt) return;
  const uint32_t pos = blockIdx.x * 256 + threadIdx.x;
  bool tie = false;
  uint32_t root = 0u;
  uint64_t pair = kOrientNoPair;
  if (pos < cnt) {
    const uint64_t w = S.lane_w[pos];
    if (w != 0ull) {
      root = orient_parent(S.node[__float_as_uint(list[pos].w)]);
      tie = w == S.best_w[root];
      pair = S.lane_p[pos];
    }
  }
  wave_root_combine<1>(tie, root, pair, (int)(threadIdx.x & 63u), S.best_p);
}

__global__ __launch_bounds__(256) void orient_count_kernel(const uint32_t *__restrict__ count, const uint8_t *__restrict__ keep,
                                                           uint32_t *__restrict__ tile_count) {
  const uint32_t cnt = *count;
  if ((uint64_t)blockIdx.x * kRunTile >= cnt) return;
  tile_flag_count((int64_t)cnt, [&](int64_t j) { return keep[j] != 0; }, tile_count);
}
__global__ __launch_bounds__(1024) void orient_scan_kernel(uint32_t *__restrict__ tile_count,
                                                           const uint32_t *__restrict__ count, uint32_t *__restrict__ next) {
  const uint32_t cnt = *count;
  if (cnt == 0u) {
    if (threadIdx.x == 0) *next = 0u;
    return;
  }
  tile_scan(tile_count, (int)((cnt + kRunTile - 1) / kRunTile), next);
}
__global__ __launch_bounds__(256) void orient_write_kernel(const float4 *__restrict__ list, const uint32_t *__restrict__ count,
                                                           const uint8_t *__restrict__ keep,
                                                           const uint32_t *__restrict__ tile_offset,
                                                           float4 *__restrict__ out) {
  const uint32_t cnt = *count;
  if ((uint64_t)blockIdx.x * kRunTile >= cnt) return;
  tile_flag_write((int64_t)cnt, [&](int64_t j) { return keep[j] != 0; }, tile_offset,
                  [=](uint32_t slot, int64_t j) { out[slot] = list[j]; });
}

// A handle that holds a NaN coordinate walks a tree the NaN has put out of order, and j in N(i) no longer means i in
// N(j): a component may not see an edge that another component takes into it, and first choices from one side only
// could close a cycle of any length.  There every root's choice is offered to the root it points at as well (the same
// two steps, then the better of the own and the offered choice stays).  After that a choice f_A into B was either A's
// own, which B was offered, or X's own into A, which X kept or bettered: round any cycle the choices cannot get worse,
// so they are one edge, the mutual pair, as on every other handle -- where the offer changes nothing and is not run.
// kStep: 0 the weights, 1 the pair words (the last bit turned: the edge as the other side holds it), 2 the better stays.
template <int kStep>
__global__ __launch_bounds__(256) void orient_offer_kernel(const uint32_t *__restrict__ count, int64_t n, OrientState S) {
  if (*count == 0u) return;
  const int64_t r64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r64 >= n) return;
  const uint32_t r = (uint32_t)r64;
  if (kStep == 2) {
    const OrientEdge own{S.best_w[r], S.best_p[r]}, in{S.in_w[r], S.in_p[r]};
    if (orient_before(in, own)) {
      S.best_w[r] = in.weight;
      S.best_p[r] = in.pair;
    }
    return;
  }
  const uint64_t w = S.best_w[r];
  if (w == 0ull) return;
  const uint64_t e = S.best_p[r];
  const uint32_t x = orient_parent(S.node[orient_pair_other(e)]);
  if (kStep == 0) {
    if (w > __atomic_load_n(S.in_w + x, __ATOMIC_RELAXED)) atomicMax(S.in_w + x, (unsigned long long)w);
  } else if (w == S.in_w[x]) {
    const uint64_t turned = e ^ 1ull;
    if (turned < __atomic_load_n(S.in_p + x, __ATOMIC_RELAXED)) atomicMin(S.in_p + x, (unsigned long long)turned);
  }
}

// one lane per id; a root with a choice hooks (the comment at the head of the file says why this is safe)
__global__ __launch_bounds__(256) void orient_hook_kernel(const uint32_t *__restrict__ count, int64_t n, OrientState S) {
  if (*count == 0u) return;
  const int64_t r64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r64 >= n) return;
  const uint32_t r = (uint32_t)r64;
  if (S.best_w[r] == 0ull) return;
  const uint64_t e = S.best_p[r];
  const uint32_t a = orient_pair_mine(e), b = orient_pair_other(e);
  const uint32_t wa = a == r ? orient_node(r, 0u) : S.node[a];
  const uint32_t wb = node_load(S.node + b);
  const uint32_t x = orient_parent(wb);
  if (x == r) return;  // the other side chose this edge too and has hooked under me
  if (S.best_w[x] != 0ull && orient_same_edge(S.best_p[x], e) && r < x) return;  // it will hook under me
  const float *na = S.normals + 3 * (size_t)a, *nb = S.normals + 3 * (size_t)b;
  const uint32_t s = orient_s(orient_c(na[0], na[1], na[2], nb[0], nb[1], nb[2]));
  node_store(S.node + r, orient_hook_word(x, orient_parity(wa), s, orient_parity(wb)));
}

// one lane per id: jump until the word names a root; the choice words back to "none" for the next round
__global__ __launch_bounds__(256) void orient_jump_kernel(const uint32_t *__restrict__ count, int64_t n, OrientState S) {
  if (*count == 0u) return;
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i64 >= n) return;
  const uint32_t i = (uint32_t)i64;
  if (S.best_w[i] != 0ull) {
    S.best_w[i] = 0ull;
    S.best_p[i] = kOrientNoPair;
    if (S.in_w) {
      S.in_w[i] = 0ull;
      S.in_p[i] = kOrientNoPair;
    }
  }
  uint32_t w = node_load(S.node + i);
  for (;;) {
    const uint32_t p = orient_parent(w);
    if (p == i) break;
    const uint32_t wp = node_load(S.node + p);
    if (orient_parent(wp) == p) break;
    w = orient_jump(w, wp);
    node_store(S.node + i, w);
  }
}

// roots -> the smallest member id
__global__ __launch_bounds__(256) void orient_minid_kernel(int64_t n, OrientState S) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i64 < n && S.ok[i64] != 0;
  const uint32_t root = valid ? orient_parent(S.node[i64]) : 0u;
  wave_root_flush<false>(valid, root, 0u, (uint32_t)i64, (int)(threadIdx.x & 63u), __ballot(valid), nullptr, S.min_id);
}

// a member's parity relative to its component's smallest member (both words name the same root)
__device__ __forceinline__ uint32_t orient_pi(const OrientState &S, const uint32_t i, const uint32_t root) {
  return orient_parity(S.node[i]) ^ orient_parity(S.node[S.min_id[root]]);
}

// mode 1: the anchor key; mode 2: the vote; per component
template <int kMode>
__global__ __launch_bounds__(256) void orient_member_kernel(QuerySource Q, OrientState S, float rx, float ry, float rz) {
  const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool valid = false;
  uint32_t root = 0u;
  uint64_t word = 0ull;
  if (pos < Q.nq) {
    int64_t i64 = 0;
    float px, py, pz;
    read_query(Q, pos, i64, px, py, pz);
    const uint32_t i = (uint32_t)i64;
    if (S.ok[i]) {
      valid = true;
      root = orient_parent(S.node[i]);
      if (kMode == 1) {
        word = orient_anchor_key(orient_height(px, py, pz, rx, ry, rz), i);
      } else {
        const float *nm = S.normals + 3 * (size_t)i;
        word = orient_vote_word(orient_vote(nm[0], nm[1], nm[2], orient_pi(S, i, root), px, py, pz, rx, ry, rz));
      }
    }
  }
  wave_root_combine<(kMode == 1 ? 0 : 2)>(valid, root, word, (int)(threadIdx.x & 63u), S.sig);
}

// one lane per id: a root with members gets its sign; the components and the open ones are counted
__global__ __launch_bounds__(256) void orient_sign_kernel(int64_t n, int32_t mode, OrientState S, float rx, float ry, float rz) {
  const int64_t r64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool comp = false, open = false;
  if (r64 < n) {
    const uint32_t r = (uint32_t)r64;
    comp = S.min_id[r] != 0xffffffffu;
    open = S.best_w[r] != 0ull;
    if (comp) {
      uint32_t sigma = 0u;
      if (mode == 1) {
        const uint32_t a = orient_anchor_id(S.sig[r]);
        const float *na = S.normals + 3 * (size_t)a;
        sigma = orient_anchor_sigma(na[0], na[1], na[2], orient_pi(S, a, r), rx, ry, rz);
      } else if (mode == 2) {
        sigma = orient_vote_sigma(S.sig[r]);
      }
      S.sigma[r] = (uint8_t)sigma;
    }
  }
  const unsigned long long cb = __ballot(comp), ob = __ballot(open);
  if ((threadIdx.x & 63u) == 0u) {
    if (cb) atomicAdd(S.totals, (uint32_t)__popcll(cb));
    if (ob) atomicAdd(S.totals + 1, (uint32_t)__popcll(ob));
  }
}

// the outputs; in place over the normals is fine: a lane reads and writes its own point's only
__global__ __launch_bounds__(256) void orient_out_kernel(int64_t n, OrientState S, uint32_t *normals_out,
                                                         uint8_t *__restrict__ flipped, int32_t *__restrict__ component,
                                                         int32_t *__restrict__ n_components, int32_t *__restrict__ n_open) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i64 == 0) {
    *n_components = (int32_t)S.totals[0];
    *n_open = (int32_t)S.totals[1];
  }
  if (i64 >= n) return;
  const uint32_t i = (uint32_t)i64;
  uint32_t flip = 0u;
  int32_t comp = -1;
  if (S.ok[i]) {
    const uint32_t root = orient_parent(S.node[i]);
    flip = orient_pi(S, i, root) ^ (uint32_t)S.sigma[root];
    comp = (int32_t)S.min_id[root];
  }
  if (flipped) flipped[i] = (uint8_t)flip;
  if (component) component[i] = comp;
  if (normals_out) {
    const uint32_t *in = (const uint32_t *)S.normals + 3 * (size_t)i;
    const uint32_t b0 = in[0], b1 = in[1], b2 = in[2];
    uint32_t *o = normals_out + 3 * (size_t)i;
    o[0] = orient_flip_bits(b0, flip);
    o[1] = orient_flip_bits(b1, flip);
    o[2] = orient_flip_bits(b2, flip);
  }
}

namespace {

struct OrientRun {
  const pcgx_kdtree *t;
  int64_t n;
  RangeSrc src;
  TreeView tv;
  XTreeView xv;
  QuerySource Q;
  size_t stack_bytes;
  float bound;
  OrientState S;
  float4 *list[2];
  uint32_t *tile_count;
  uint32_t *words;  // the active count before round k, k = 0 .. rounds
};

template <int kSrc>
void orient_edge_launch(const OrientRun &r, const float4 *list, const uint32_t *count, hipStream_t st) {
  const dim3 grid(xcd_grid((unsigned)((r.n + kOrientBlock - 1) / kOrientBlock))), block(kOrientBlock);
  const GridView g = kSrc == kRangeGrid ? r.t->grid : GridView{};
  hipLaunchKernelGGL(orient_edge_kernel<kSrc>, grid, block, r.stack_bytes, st, g, r.tv, r.xv, list, count, r.bound, r.S,
                     xwalk_guard(r.n));
}
void orient_edge_enqueue(const OrientRun &r, const float4 *list, const uint32_t *count, hipStream_t st) {
  if (r.src == kRangeXWalk) orient_edge_launch<kRangeXWalk>(r, list, count, st);
  else if (r.src == kRangeGrid) orient_edge_launch<kRangeGrid>(r, list, count, st);
  else orient_edge_launch<kRangeWalk>(r, list, count, st);
}

void orient_offer_enqueue(const uint32_t *count, int64_t n, const OrientState &S, hipStream_t st) {
  const dim3 nb((unsigned)((n + 255) / 256)), b256(256);
  hipLaunchKernelGGL(orient_offer_kernel<0>, nb, b256, 0, st, count, n, S);
  hipLaunchKernelGGL(orient_offer_kernel<1>, nb, b256, 0, st, count, n, S);
  hipLaunchKernelGGL(orient_offer_kernel<2>, nb, b256, 0, st, count, n, S);
}

}  // namespace

// Len() > 0, everything device resident; temporaries from ctx().arena, which the caller has begun.  d_active (may be
// nullptr): uint32 [rounds + 1], the active points before each round and after the last.
pcgx_status orient_enqueue(const pcgx_kdtree *t, float radius, const float *d_normals, int32_t mode, const float *ref3,
                           int32_t rounds, float *d_normals_out, uint8_t *d_flipped, int32_t *d_component,
                           int32_t *d_n_components, int32_t *d_n_open, uint32_t *d_active, hipStream_t st) {
  Arena &ar = ctx().arena;
  OrientRun r{};
  r.t = t;
  r.n = t->n;
  r.src = range_source(t);  // as pcgx_kdtree_range_count takes it
  if (r.src == kRangeXWalk) PCGX_TRY(xtree_view(t, &r.xv, st));
  r.tv = t->view();
  PCGX_TRY(query_source(t, r.src, nullptr, r.n, &r.Q, st));
  r.stack_bytes = r.src == kRangeXWalk ? xwalk_stack_bytes(r.xv, kOrientBlock)
                  : r.src == kRangeGrid ? 0 : walk_stack_bytes(r.tv, kOrientBlock);
  r.bound = radius * radius;
  const size_t n = (size_t)r.n;
  OrientState &S = r.S;
  S.normals = d_normals;
  PCGX_TRY(ar.alloc_n(n, &S.best_w));
  PCGX_TRY(ar.alloc_n(n, &S.best_p));
  PCGX_TRY(ar.alloc_n(n, &S.lane_w));
  PCGX_TRY(ar.alloc_n(n, &S.lane_p));
  PCGX_TRY(ar.alloc_n(n, &S.sig));
  if (t->has_nan) {
    PCGX_TRY(ar.alloc_n(n, &S.in_w));
    PCGX_TRY(ar.alloc_n(n, &S.in_p));
  }
  PCGX_TRY(ar.alloc_n(n, &r.list[0]));
  PCGX_TRY(ar.alloc_n(n, &r.list[1]));
  PCGX_TRY(ar.alloc_n(n, &S.node));
  PCGX_TRY(ar.alloc_n(n, &S.min_id));
  PCGX_TRY(ar.alloc_n((n + kRunTile - 1) / kRunTile, &r.tile_count));
  PCGX_TRY(ar.alloc_n((size_t)rounds + 1, &r.words));
  PCGX_TRY(ar.alloc_n(2, &S.totals));
  PCGX_TRY(ar.alloc_n(n, &S.ok));
  PCGX_TRY(ar.alloc_n(n, &S.keep));
  PCGX_TRY(ar.alloc_n(n, &S.sigma));
  const dim3 nb((unsigned)((n + 255) / 256)), b256(256);
  const unsigned ntiles = (unsigned)((n + kRunTile - 1) / kRunTile);
  hipLaunchKernelGGL(orient_prep_kernel, nb, b256, 0, st, r.Q, S, r.list[0], r.words);
  if (S.in_w) {  // who is in its own neighbourhood; the offers of this pass mean nothing
    orient_edge_enqueue(r, r.list[0], r.words, st);
    PCGX_HIP_TRY(hipMemsetAsync(S.best_w, 0, n * sizeof(unsigned long long), st));
  }
  for (int32_t k = 0; k < rounds; k++) {
    const float4 *cur = r.list[k & 1];
    float4 *nxt = r.list[(k + 1) & 1];
    const uint32_t *count = r.words + k;
    orient_edge_enqueue(r, cur, count, st);
    hipLaunchKernelGGL(orient_tie_kernel, nb, b256, 0, st, cur, count, S);
    hipLaunchKernelGGL(orient_count_kernel, dim3(ntiles), b256, 0, st, count, (const uint8_t *)S.keep, r.tile_count);
    hipLaunchKernelGGL(orient_scan_kernel, dim3(1), dim3(1024), 0, st, r.tile_count, count, r.words + k + 1);
    hipLaunchKernelGGL(orient_write_kernel, dim3(ntiles), b256, 0, st, cur, count, (const uint8_t *)S.keep,
                       (const uint32_t *)r.tile_count, nxt);
    if (S.in_w) orient_offer_enqueue(count, r.n, S, st);
    hipLaunchKernelGGL(orient_hook_kernel, nb, b256, 0, st, count, r.n, S);
    hipLaunchKernelGGL(orient_jump_kernel, nb, b256, 0, st, count, r.n, S);
  }
  // the roots that still have a leaving edge: the next round's offers, taken by nobody
  orient_edge_enqueue(r, r.list[rounds & 1], r.words + rounds, st);
  if (S.in_w) {
    hipLaunchKernelGGL(orient_tie_kernel, nb, b256, 0, st, r.list[rounds & 1], r.words + rounds, S);
    orient_offer_enqueue(r.words + rounds, r.n, S, st);
  }
  hipLaunchKernelGGL(orient_minid_kernel, nb, b256, 0, st, r.n, S);
  const float rx = mode ? ref3[0] : 0.0f, ry = mode ? ref3[1] : 0.0f, rz = mode ? ref3[2] : 0.0f;
  if (mode == 1) hipLaunchKernelGGL(orient_member_kernel<1>, nb, b256, 0, st, r.Q, S, rx, ry, rz);
  if (mode == 2) hipLaunchKernelGGL(orient_member_kernel<2>, nb, b256, 0, st, r.Q, S, rx, ry, rz);
  hipLaunchKernelGGL(orient_sign_kernel, nb, b256, 0, st, r.n, mode, S, rx, ry, rz);
  hipLaunchKernelGGL(orient_out_kernel, nb, b256, 0, st, r.n, S, (uint32_t *)d_normals_out, d_flipped, d_component,
                     d_n_components, d_n_open);
  PCGX_HIP_TRY(hipGetLastError());
  if (d_active)
    PCGX_HIP_TRY(hipMemcpyAsync(d_active, r.words, ((size_t)rounds + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  return PCGX_OK;
}

}  // namespace pcgx

using namespace pcgx;

namespace {

pcgx_status orient_check(const char *fn, const pcgx_kdtree *t, float radius, const void *normals, int32_t mode,
                         const float *ref3, int32_t max_rounds, const void *normals_out, const void *flipped,
                         const void *n_components, const void *n_open) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!(radius > 0.0f && radius < __builtin_inff())) return fail(PCGX_E_INVALID, "%s: radius must be finite and > 0", fn);
  if (mode < 0 || mode > 2) return fail(PCGX_E_INVALID, "%s: mode must be 0, 1 or 2", fn);
  if (mode != 0) {
    if (!ref3) return fail(PCGX_E_INVALID, "%s: this mode needs a direction or a viewpoint", fn);
    for (int k = 0; k < 3; k++)
      if (!cluster_finite(ref3[k])) return fail(PCGX_E_INVALID, "%s: the direction or viewpoint must be finite", fn);
  }
  if (max_rounds < 0) return fail(PCGX_E_INVALID, "%s: max_rounds must be >= 0", fn);
  if (t->n > (int64_t)kOrientMaxId) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 2 points", fn);
  if (!n_components || !n_open) return fail(PCGX_E_INVALID, "%s: NULL n_components or n_open", fn);
  if (t->n > 0 && (!normals || (!normals_out && !flipped)))
    return fail(PCGX_E_INVALID, "%s: NULL normals, or neither normals_out nor flipped", fn);
  return PCGX_OK;
}

pcgx_status orient_dev(const char *fn, const pcgx_kdtree *t, float radius, const float *d_normals, int32_t mode,
                       const float *ref3, int32_t max_rounds, float *d_normals_out, uint8_t *d_flipped,
                       int32_t *d_component, int32_t *d_n_components, int32_t *d_n_open, uint32_t *d_active, void *stream) {
  PCGX_TRY(orient_check(fn, t, radius, d_normals, mode, ref3, max_rounds, d_normals_out, d_flipped, d_n_components,
                        d_n_open));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  if (t->n == 0) {
    PCGX_HIP_TRY(hipMemsetAsync(d_n_components, 0, sizeof(int32_t), st));
    PCGX_HIP_TRY(hipMemsetAsync(d_n_open, 0, sizeof(int32_t), st));
    return PCGX_OK;
  }
  PCGX_TRY(ctx().arena.begin(st));
  return orient_enqueue(t, radius, d_normals, mode, ref3, max_rounds > 0 ? max_rounds : orient_full_rounds(t->n),
                        d_normals_out, d_flipped, d_component, d_n_components, d_n_open, d_active, st);
}

}  // namespace

extern "C" int32_t pcgx_orient_full_rounds(int64_t n) { return n > 0 ? orient_full_rounds(n) : 0; }
extern "C" int32_t pcgx_orient_active_list(void) { return kOrientActiveList ? 1 : 0; }

extern "C" pcgx_status pcgx_kdtree_orient_normals_dev(const pcgx_kdtree *t, float radius, const float *d_normals,
                                                      int32_t mode, const float *ref3, int32_t max_rounds,
                                                      float *d_normals_out, uint8_t *d_flipped, int32_t *d_component,
                                                      int32_t *d_n_components, int32_t *d_n_open, void *stream) {
  PCGX_API_LOCK();
  return orient_dev("pcgx_kdtree_orient_normals_dev", t, radius, d_normals, mode, ref3, max_rounds, d_normals_out,
                    d_flipped, d_component, d_n_components, d_n_open, nullptr, stream);
}

extern "C" pcgx_status pcgx_kdtree_orient_normals_probe_dev(const pcgx_kdtree *t, float radius, const float *d_normals,
                                                            int32_t mode, const float *ref3, int32_t max_rounds,
                                                            float *d_normals_out, uint8_t *d_flipped,
                                                            int32_t *d_n_components, int32_t *d_n_open,
                                                            uint32_t *d_active, void *stream) {
  PCGX_API_LOCK();
  return orient_dev("pcgx_kdtree_orient_normals_probe_dev", t, radius, d_normals, mode, ref3, max_rounds, d_normals_out,
                    d_flipped, nullptr, d_n_components, d_n_open, d_active, stream);
}

extern "C" pcgx_status pcgx_kdtree_orient_normals(const pcgx_kdtree *t, float radius, const float *normals, int32_t mode,
                                                  const float *ref3, float *normals_out, uint8_t *flipped,
                                                  int64_t *component, int64_t *n_components, int64_t *n_open) {
  PCGX_API_CALL();
  PCGX_TRY(orient_check("pcgx_kdtree_orient_normals", t, radius, normals, mode, ref3, 0, normals_out, flipped,
                        n_components, n_open));
  const int64_t n = t->n;
  if (n == 0) {
    *n_components = 0;
    *n_open = 0;
    return PCGX_OK;
  }
  PCGX_TRY(ensure_init());
  // always on the device: the rounds are the kernels', not a host restatement; enough rounds to finish for certain
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_nrm = nullptr;
  uint8_t *d_flip = nullptr;
  int32_t *d_comp = nullptr, *d_counts = nullptr;  // d_comp: [n]; d_counts: {components, open}
  PCGX_TRY(ha.alloc_n((size_t)n * 3, &d_nrm));
  PCGX_TRY(staged_upload(d_nrm, normals, (size_t)n * 12, st));
  PCGX_TRY(ha.alloc_n(2, &d_counts));
  if (component) PCGX_TRY(ha.alloc_n((size_t)n, &d_comp));
  if (flipped) PCGX_TRY(ha.alloc_n((size_t)n, &d_flip));
  PCGX_TRY(pcgx_kdtree_orient_normals_dev(t, radius, d_nrm, mode, ref3, 0, normals_out ? d_nrm : nullptr, d_flip, d_comp,
                                          d_counts, d_counts + 1, st));
  if (normals_out) PCGX_TRY(staged_download(normals_out, d_nrm, (size_t)n * 12, st));
  if (flipped) PCGX_TRY(staged_download(flipped, d_flip, (size_t)n, st));
  int32_t hc[2] = {0, 0};
  PCGX_TRY(staged_download(hc, d_counts, sizeof hc, st));
  *n_components = hc[0];
  *n_open = hc[1];
  if (component) {
    RawVector<int32_t> h((size_t)n);
    PCGX_TRY(staged_download(h.data(), d_comp, (size_t)n * 4, st));
    for (int64_t i = 0; i < n; i++) component[i] = h[(size_t)i];
  }
  return PCGX_OK;
}
