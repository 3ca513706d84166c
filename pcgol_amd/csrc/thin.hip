// thin.hip -- minimum-distance subsampling over a tree's own points: a maximal set of ORIGINAL points no two of which
// are within the radius, and for every dropped point the kept point that stands for it (extension: no reference parity;
// include/pcgx.h, "minimum-distance subsampling").
//
// The kept set is what sequential greedy selection in priority order keeps, the lexicographically first maximal
// independent set of the radius graph.  It is computed in parallel rounds; a round decides an undecided point from the
// FINAL states of its neighbours that come before it, so every schedule reaches the same set, and because a round reads
// only what the round before left, the states after R rounds are a property of the point set too.
//   thin_prep_kernel      by-id state (UNDECIDED, or INELIGIBLE for a NaN score), owner -2, the kept flags zero, and the
//                         first undecided list {x, y, z, bits(id)} in the order query_source has (read_query serves it).
//   thin_round_kernel     one more consumer of the shared enumeration (radius_visit.h), one undecided point per lane.
//                         Per member: its state byte and its priority by id (the score's 4 bytes, or shape_mix
//                         recomputed: no load), and three bits -- a member before me is KEPT, one is UNDECIDED, I met
//                         myself (a deleted id or a non-finite coordinate never does, and becomes INELIGIBLE in round 1:
//                         no flags array).  The decision goes into a byte per LIST POSITION, never into the by-id states
//                         the other lanes are reading.
//   thin_commit_kernel    the decisions into the by-id states and the kept flags, and the tile counts of the still
//   thin_scan_kernel      undecided; their scan, whose total is the next round's count word; the still undecided
//   thin_write_kernel     records, in order, into the other list buffer (bucket_grid.h's tile compaction).
//   thin_owner_kernel     one lane per point in the handle's order; a DROPPED one enumerates and keeps the smallest
//                         (DistSq, id) among its KEPT members.
// Every round's kernels read the undecided count from a device word and return at once when it is zero; nothing waits
// on another workgroup; nothing is read back by the device form.  Of a fat row's shares the bits are combined over the
// wave by ballots and the owner's minimum by shuffles, and the owner lane merges them.
#include <math.h>
#include <stdlib.h>

#include "bucket_grid.h"
#include "radius_visit.h"
#include "thin_terms.h"

namespace pcgx {

// keypoints.hip
pcgx_status flags_to_ids_enqueue(const uint8_t *d_flag, int64_t n, uint32_t *tile_count, int32_t *d_ids, int32_t *d_n_ids,
                                 hipStream_t st);

constexpr int kThinBlock = kRangeWalkBlock;  // one wave per workgroup: the walks' LDS frame stacks are [level][64]

__global__ __launch_bounds__(256) void thin_prep_kernel(QuerySource Q, const float *__restrict__ score,
                                                        uint8_t *__restrict__ state, uint8_t *__restrict__ kept,
                                                        int32_t *__restrict__ owner, float4 *__restrict__ list,
                                                        uint32_t *__restrict__ count) {
  const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pos == 0) *count = (uint32_t)Q.nq;
  if (pos >= Q.nq) return;
  int64_t i = 0;
  float qx, qy, qz;
  read_query(Q, pos, i, qx, qy, qz);
  list[pos] = make_float4(qx, qy, qz, __uint_as_float((uint32_t)i));
  state[i] = thin_score_ok(score != nullptr, score ? score[i] : 0.0f) ? kThinUndecided : kThinIneligible;
  kept[i] = 0;
  if (owner) owner[i] = kThinNotRun;
}

// the three bits of one undecided point
struct ThinBits {
  bool kept_before, undecided_before, met;

  // the record p, inside the bound of point i (score si); kScore: score mode
  template <bool kScore>
  __device__ __forceinline__ void take(const uint8_t *__restrict__ state, const float *__restrict__ score,
                                       const uint32_t seed, const float4 &p, const float si, const uint32_t i) {
    const uint32_t j = __float_as_uint(p.w);
    if (j == i) {
      met = true;
      return;
    }
    if (kept_before) return;  // decided: DROPPED
    const uint8_t sj = state[j];
    if (sj != kThinKept && sj != kThinUndecided) return;
    if (!thin_before(kScore, seed, kScore ? score[j] : 0.0f, j, si, i)) return;
    if (sj == kThinKept) kept_before = true;
    else undecided_before = true;
  }
};

template <int kSrc, bool kScore>
__global__ __launch_bounds__(kThinBlock) void thin_round_kernel(GridView g, TreeView tv, XTreeView xv,
                                                                const float4 *__restrict__ list,
                                                                const uint32_t *__restrict__ count, float bound,
                                                                const float *__restrict__ score, uint32_t seed,
                                                                const uint8_t *__restrict__ state,
                                                                uint8_t *__restrict__ dec, int64_t guard) {
  extern __shared__ uint32_t s_stack[];
  const uint32_t cnt = *count;
  if (cnt == 0u) return;
  const uint32_t n_tiles = (cnt + kThinBlock - 1) / kThinBlock;
  if ((blockIdx.x >> 3) >= (n_tiles + 7u) / 8u) return;  // (xcd_tile beyond an XCD's share would name another's tile)
  const uint32_t tile = xcd_tile(blockIdx.x, n_tiles);
  if (tile >= n_tiles) return;
  const uint32_t pos = tile * kThinBlock + threadIdx.x;
  const bool live = pos < cnt;
  uint32_t i = 0u;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f, si = 0.0f;
  bool cand = false;
  if (live) {
    const float4 r = list[pos];
    i = __float_as_uint(r.w);
    qx = r.x; qy = r.y; qz = r.z;
    if (kScore) si = score[i];
    cand = state[i] == kThinUndecided;  // (round 1's list holds the NaN scores too)
  }
  ThinBits b{false, false, false};
  const int lane = (int)(threadIdx.x & 63u);
  radius_visit<kSrc>(
      RadiusViews{g, tv, xv, guard}, s_stack + threadIdx.x, kThinBlock, qx, qy, qz, bound, cand,
      [&](const float4 &p, float) { b.template take<kScore>(state, score, seed, p, si, i); },
      [&](int owner, float, float, float, auto rows) {  // the three bits, combined over the wave by ballots
        const float osi = __shfl(si, owner);
        const uint32_t oi = __shfl(i, owner);
        ThinBits part{false, false, false};
        rows([&](const float4 &p, float) { part.template take<kScore>(state, score, seed, p, osi, oi); });
        const bool any_kept = __ballot(part.kept_before) != 0ull, any_und = __ballot(part.undecided_before) != 0ull,
                   any_met = __ballot(part.met) != 0ull;
        if (lane == owner) {
          b.kept_before = b.kept_before || any_kept;
          b.undecided_before = b.undecided_before || any_und;
          b.met = b.met || any_met;
        }
      });
  if (!live) return;
  dec[pos] = thin_decide(cand && b.met, b.kept_before, b.undecided_before);
}

// The decisions of the round into the by-id states (the round kernel is done reading them), counting the still undecided
// per tile.  flag(j) is called once per position: the commit rides on it.
__global__ __launch_bounds__(256) void thin_commit_kernel(const float4 *__restrict__ list, const uint32_t *__restrict__ count,
                                                          const uint8_t *__restrict__ dec, uint8_t *__restrict__ state,
                                                          uint8_t *__restrict__ kept, uint32_t *__restrict__ tile_count) {
  const uint32_t cnt = *count;
  if ((uint64_t)blockIdx.x * kRunTile >= cnt) return;
  tile_flag_count(
      (int64_t)cnt,
      [&](int64_t j) {
        const uint8_t d = dec[j];
        if (d == kThinUndecided) return true;
        const uint32_t id = __float_as_uint(list[j].w);
        state[id] = d;
        if (d == kThinKept) kept[id] = 1;
        return false;
      },
      tile_count);
}
__global__ __launch_bounds__(1024) void thin_scan_kernel(uint32_t *__restrict__ tile_count,
                                                         const uint32_t *__restrict__ count, uint32_t *__restrict__ next) {
  const uint32_t cnt = *count;
  if (cnt == 0u) {
    if (threadIdx.x == 0) *next = 0u;
    return;
  }
  tile_scan(tile_count, (int)((cnt + kRunTile - 1) / kRunTile), next);
}
__global__ __launch_bounds__(256) void thin_write_kernel(const float4 *__restrict__ list, const uint32_t *__restrict__ count,
                                                         const uint8_t *__restrict__ dec,
                                                         const uint32_t *__restrict__ tile_offset,
                                                         float4 *__restrict__ out) {
  const uint32_t cnt = *count;
  if ((uint64_t)blockIdx.x * kRunTile >= cnt) return;
  tile_flag_write((int64_t)cnt, [&](int64_t j) { return dec[j] == kThinUndecided; }, tile_offset,
                  [=](uint32_t slot, int64_t j) { out[slot] = list[j]; });
}

// the smallest (DistSq, id) among a dropped point's kept members
struct ThinBest {
  float d;
  uint32_t id;

  __device__ __forceinline__ void take(const uint8_t *__restrict__ state, const float4 &p, const float dist) {
    const uint32_t j = __float_as_uint(p.w);
    if (state[j] != kThinKept) return;
    if (thin_owner_beats(dist, j, d, id)) {
      d = dist;
      id = j;
    }
  }
  __device__ __forceinline__ void merge(const float od, const uint32_t oid) {
    if (thin_owner_beats(od, oid, d, id)) {
      d = od;
      id = oid;
    }
  }
};

template <int kSrc>
__global__ __launch_bounds__(kThinBlock) void thin_owner_kernel(GridView g, TreeView tv, XTreeView xv, QuerySource Q,
                                                                const uint32_t *__restrict__ n_left, float bound,
                                                                const uint8_t *__restrict__ state,
                                                                int32_t *__restrict__ owner, int64_t guard) {
  extern __shared__ uint32_t s_stack[];
  if (*n_left != 0u) return;  // not the contract's states yet: owner stays -2
  const uint32_t n_tiles = (uint32_t)((Q.nq + kThinBlock - 1) / kThinBlock);
  const int64_t pos = (int64_t)xcd_tile(blockIdx.x, n_tiles) * kThinBlock + threadIdx.x;
  const bool live = pos < Q.nq;
  int64_t i64 = 0;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  uint8_t si = kThinIneligible;
  if (live) {
    read_query(Q, pos, i64, qx, qy, qz);
    si = state[i64];
  }
  ThinBest b{__builtin_inff(), 0xffffffffu};
  const int lane = (int)(threadIdx.x & 63u);
  radius_visit<kSrc>(
      RadiusViews{g, tv, xv, guard}, s_stack + threadIdx.x, kThinBlock, qx, qy, qz, bound, live && si == kThinDropped,
      [&](const float4 &p, float d) { b.take(state, p, d); },
      [&](int row_owner, float, float, float, auto rows) {  // the minimum, combined over the wave by shuffles
        ThinBest part{__builtin_inff(), 0xffffffffu};
        rows([&](const float4 &p, float d) { part.take(state, p, d); });
        for (int o = 32; o > 0; o >>= 1) part.merge(__shfl_xor(part.d, o), __shfl_xor(part.id, o));
        if (lane == row_owner) b.merge(part.d, part.id);
      });
  if (!live) return;
  owner[i64] = si == kThinKept ? (int32_t)i64 : (si == kThinDropped && b.id != 0xffffffffu) ? (int32_t)b.id : kThinNoOwner;
}

// One call's state between its enqueues: the host form runs batches of rounds on it until the count word is zero.
struct ThinRun {
  const pcgx_kdtree *t;
  int64_t n;
  RangeSrc src;
  TreeView tv;
  XTreeView xv;
  QuerySource Q;
  size_t stack_bytes;
  float bound;
  uint32_t seed;
  const float *score;
  uint8_t *state, *kept, *dec;
  float4 *list[2];
  uint32_t *tile_count;
  const uint32_t *count;  // the undecided count as the last enqueued round leaves it
  int64_t rounds;         // enqueued so far (their parity says which list is current)
  int64_t upper;          // a bound of *count known on the host (Len(), or what the host form read)
};

// Len() > 0, everything device resident; temporaries from ctx().arena, which the caller has begun.  d_kept: the kept
// flags by id where the caller wants them (the filters), else nullptr.
pcgx_status thin_prepare(const pcgx_kdtree *t, float radius, uint32_t seed, const float *d_score, uint8_t *d_kept,
                         int32_t *d_owner, ThinRun *run, hipStream_t st) {
  Arena &ar = ctx().arena;
  ThinRun &r = *run;
  r = ThinRun{};
  r.t = t;
  r.n = t->n;
  r.src = range_source(t);  // as pcgx_kdtree_range_count takes it
  if (r.src == kRangeXWalk) PCGX_TRY(xtree_view(t, &r.xv, st));
  r.tv = t->view();
  PCGX_TRY(query_source(t, r.src, nullptr, r.n, &r.Q, st));
  r.stack_bytes = r.src == kRangeXWalk ? xwalk_stack_bytes(r.xv, kThinBlock)
                  : r.src == kRangeGrid ? 0 : walk_stack_bytes(r.tv, kThinBlock);
  r.bound = radius * radius;
  r.seed = seed;
  r.score = d_score;
  r.kept = d_kept;
  const size_t n = (size_t)r.n;
  uint32_t *count = nullptr;
  PCGX_TRY(ar.alloc_n(n, &r.state));
  if (!r.kept) PCGX_TRY(ar.alloc_n(n, &r.kept));
  PCGX_TRY(ar.alloc_n(n, &r.dec));
  PCGX_TRY(ar.alloc_n(n, &r.list[0]));
  PCGX_TRY(ar.alloc_n(n, &r.list[1]));
  PCGX_TRY(ar.alloc_n((n + kRunTile - 1) / kRunTile, &r.tile_count));
  PCGX_TRY(ar.alloc_n(1, &count));
  hipLaunchKernelGGL(thin_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, r.Q, d_score, r.state, r.kept,
                     d_owner, r.list[0], count);
  PCGX_HIP_TRY(hipGetLastError());
  r.count = count;
  r.upper = r.n;
  return PCGX_OK;
}

template <int kSrc, bool kScore>
void thin_round_launch(const ThinRun &r, const float4 *list, hipStream_t st) {
  const dim3 grid(xcd_grid((unsigned)((r.upper + kThinBlock - 1) / kThinBlock))), block(kThinBlock);
  const GridView g = kSrc == kRangeGrid ? r.t->grid : GridView{};
  hipLaunchKernelGGL((thin_round_kernel<kSrc, kScore>), grid, block, r.stack_bytes, st, g, r.tv, r.xv, list, r.count, r.bound,
                     r.score, r.seed, (const uint8_t *)r.state, r.dec, xwalk_guard(r.n));
}
template <int kSrc>
void thin_round_launch(const ThinRun &r, const float4 *list, hipStream_t st) {
  if (r.score) thin_round_launch<kSrc, true>(r, list, st);
  else thin_round_launch<kSrc, false>(r, list, st);
}

// `rounds` more rounds: four launches each, every one a no-op once the count word is zero.
pcgx_status thin_rounds_enqueue(ThinRun *run, int64_t rounds, hipStream_t st) {
  ThinRun &r = *run;
  uint32_t *words = nullptr;  // the counts these rounds leave
  PCGX_TRY(ctx().arena.alloc_n((size_t)rounds, &words));
  const unsigned ntiles = (unsigned)((r.upper + kRunTile - 1) / kRunTile);
  for (int64_t k = 0; k < rounds; k++, r.rounds++) {
    const float4 *cur = r.list[r.rounds & 1];
    float4 *nxt = r.list[(r.rounds + 1) & 1];
    if (r.src == kRangeXWalk) thin_round_launch<kRangeXWalk>(r, cur, st);
    else if (r.src == kRangeGrid) thin_round_launch<kRangeGrid>(r, cur, st);
    else thin_round_launch<kRangeWalk>(r, cur, st);
    hipLaunchKernelGGL(thin_commit_kernel, dim3(ntiles), dim3(256), 0, st, cur, r.count, (const uint8_t *)r.dec, r.state,
                       r.kept, r.tile_count);
    hipLaunchKernelGGL(thin_scan_kernel, dim3(1), dim3(1024), 0, st, r.tile_count, r.count, words + k);
    hipLaunchKernelGGL(thin_write_kernel, dim3(ntiles), dim3(256), 0, st, cur, r.count, (const uint8_t *)r.dec,
                       (const uint32_t *)r.tile_count, nxt);
    r.count = words + k;
  }
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

template <int kSrc>
void thin_owner_launch(const ThinRun &r, int32_t *d_owner, hipStream_t st) {
  const dim3 grid(xcd_grid((unsigned)((r.n + kThinBlock - 1) / kThinBlock))), block(kThinBlock);
  const GridView g = kSrc == kRangeGrid ? r.t->grid : GridView{};
  hipLaunchKernelGGL(thin_owner_kernel<kSrc>, grid, block, r.stack_bytes, st, g, r.tv, r.xv, r.Q, r.count, r.bound,
                     (const uint8_t *)r.state, d_owner, xwalk_guard(r.n));
}

// The outputs from the states as they stand: the count left, the owners (where none is left), the kept ids.
pcgx_status thin_finish_enqueue(const ThinRun &r, int32_t *d_ids, int32_t *d_n_ids, int32_t *d_owner, int32_t *d_n_left,
                                hipStream_t st) {
  if (d_n_left) PCGX_HIP_TRY(hipMemcpyAsync(d_n_left, r.count, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  if (d_owner) {
    if (r.src == kRangeXWalk) thin_owner_launch<kRangeXWalk>(r, d_owner, st);
    else if (r.src == kRangeGrid) thin_owner_launch<kRangeGrid>(r, d_owner, st);
    else thin_owner_launch<kRangeWalk>(r, d_owner, st);
    PCGX_HIP_TRY(hipGetLastError());
  }
  if (!d_ids) return PCGX_OK;
  return flags_to_ids_enqueue(r.kept, r.n, r.tile_count, d_ids, d_n_ids, st);
}

// Batches of the default number of rounds until the one count word a batch leaves reads zero.
pcgx_status thin_run_to_end(ThinRun *run, hipStream_t st) {
  for (;;) {
    PCGX_TRY(thin_rounds_enqueue(run, kThinDefaultRounds, st));
    uint32_t left = 0;
    PCGX_HIP_TRY(hipMemcpyAsync(&left, run->count, sizeof left, hipMemcpyDeviceToHost, st));
    PCGX_HIP_TRY(hipStreamSynchronize(st));
    if (left == 0u) return PCGX_OK;
    run->upper = left;
  }
}

// The kept flags of hash mode by tree id, complete (sor.hip: pcgx_thin_filter).  Begins ctx().arena; reads the count
// word back between batches.
pcgx_status thin_kept_by_id(const pcgx_kdtree *t, float radius, uint32_t seed, uint8_t *d_kept, hipStream_t st) {
  PCGX_TRY(ctx().arena.begin(st));
  ThinRun run;
  PCGX_TRY(thin_prepare(t, radius, seed, nullptr, d_kept, nullptr, &run, st));
  return thin_run_to_end(&run, st);
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kThinMaxPoints = 0x7fffffff;  // ids are int32 on the device

pcgx_status thin_check(const char *fn, const pcgx_kdtree *t, float radius, int32_t max_rounds, const void *ids,
                       const void *n_ids) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (!(radius > 0.0f && radius < __builtin_inff())) return fail(PCGX_E_INVALID, "%s: radius must be finite and > 0", fn);
  // (a bound of 0 holds nobody, not a point itself; one of +inf is no spacing)
  if (!(radius * radius > 0.0f && radius * radius < __builtin_inff()))
    return fail(PCGX_E_INVALID, "%s: the float32 square of the radius must be finite and > 0", fn);
  if (max_rounds < 0) return fail(PCGX_E_INVALID, "%s: max_rounds must be >= 0", fn);
  if (t->n > kThinMaxPoints) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points", fn);
  if (t->n > 0 && (!ids || !n_ids)) return fail(PCGX_E_INVALID, "%s: NULL ids or n_ids", fn);
  return PCGX_OK;
}

}  // namespace

extern "C" int32_t pcgx_thin_default_rounds(void) { return kThinDefaultRounds; }

extern "C" pcgx_status pcgx_kdtree_thin_dev(const pcgx_kdtree *t, float radius, uint32_t seed, const float *d_score,
                                            int32_t max_rounds, int32_t *d_ids, int32_t *d_n_ids, int32_t *d_owner,
                                            int32_t *d_n_left, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(thin_check("pcgx_kdtree_thin_dev", t, radius, max_rounds, d_ids, d_n_ids));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  if (t->n == 0) {
    if (d_n_ids) PCGX_HIP_TRY(hipMemsetAsync(d_n_ids, 0, sizeof(int32_t), st));
    if (d_n_left) PCGX_HIP_TRY(hipMemsetAsync(d_n_left, 0, sizeof(int32_t), st));
    return PCGX_OK;
  }
  PCGX_TRY(ctx().arena.begin(st));
  ThinRun run;
  PCGX_TRY(thin_prepare(t, radius, seed, d_score, nullptr, d_owner, &run, st));
  PCGX_TRY(thin_rounds_enqueue(&run, max_rounds > 0 ? max_rounds : kThinDefaultRounds, st));
  return thin_finish_enqueue(run, d_ids, d_n_ids, d_owner, d_n_left, st);
}

extern "C" pcgx_status pcgx_kdtree_thin(const pcgx_kdtree *t, float radius, uint32_t seed, const float *score, int64_t *ids,
                                        int64_t *n_ids, int64_t *owner) {
  PCGX_API_CALL();
  PCGX_TRY(thin_check("pcgx_kdtree_thin", t, radius, 0, ids, n_ids));
  const int64_t n = t->n;
  if (n == 0) {
    if (n_ids) *n_ids = 0;
    return PCGX_OK;
  }
  PCGX_TRY(ensure_init());
  // always on the device: the rounds are the kernels', not a host restatement
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  float *d_s = nullptr;
  int32_t *d_out = nullptr, *d_owner = nullptr;  // ids [n], the count; owner [n]
  if (score) {
    PCGX_TRY(ha.alloc_n((size_t)n, &d_s));
    PCGX_TRY(staged_upload(d_s, score, (size_t)n * 4, st));
  }
  PCGX_TRY(ha.alloc_n((size_t)n + 1, &d_out));
  if (owner) PCGX_TRY(ha.alloc_n((size_t)n, &d_owner));
  PCGX_TRY(ctx().arena.begin(st));
  ThinRun run;
  PCGX_TRY(thin_prepare(t, radius, seed, d_s, nullptr, d_owner, &run, st));
  PCGX_TRY(thin_run_to_end(&run, st));
  PCGX_TRY(thin_finish_enqueue(run, d_out, d_out + n, d_owner, nullptr, st));
  RawVector<int32_t> h((size_t)n + 1);
  PCGX_TRY(staged_download(h.data(), d_out, ((size_t)n + 1) * 4, st));
  for (int64_t i = 0; i < n; i++) ids[i] = h[(size_t)i];
  *n_ids = h[(size_t)n];
  if (owner) {
    PCGX_TRY(staged_download(h.data(), d_owner, (size_t)n * 4, st));
    for (int64_t i = 0; i < n; i++) owner[i] = h[(size_t)i];
  }
  return PCGX_OK;
}
