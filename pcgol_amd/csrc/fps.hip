// fps.hip -- farthest-point sampling over a tree's own points: `count` well-spread ORIGINAL points in pick order, every
// prefix a sampling of its own, and for every point the pick nearest to it (extension: no reference parity;
// include/pcgx.h, "farthest-point sampling").
//
// The picks are a dependent chain; what a pick costs is what matters.  The points are put in Morton order and cut into
// tiles of kFpsTile; a tile carries the box of its eligible members and the largest key (d, id) among its candidates.  A
// pick s leaves a tile alone whose box is at least the tile's largest d away (fps_terms.h: the lemma that makes this
// exact in float32), so late picks read a few tiles and the tiles' 40-byte summaries.
//   fps_gather_kernel   the handle's points by id out of the BFS slots of the tree that holds them (after DeletePoint:
//                       the tree over the remaining points, original ids); an id no slot names stays NaN: not eligible.
//   fps_prep_kernel     a wave per tile: records {x, y, z, bits(id)} by position, d = +inf, no owner, the candidate
//                       flags, id -> position, the tile's box and key; the first pick's key into best[0].
//   fps_pick_kernel     one launch per pick, every tile: reads pick j from the device word best[j]; a lane tests one
//                       tile's bound; a touched tile is the whole wave's, four points a lane: the strict
//                       update of d and owner, the pick itself leaves the candidates, the tile's key is formed again.  A
//                       workgroup reduces the keys of all its tiles, touched or not, into one 64-bit atomicMax on
//                       best[j + 1].  best[j] == 0 (nothing left): it returns at once and best[j + 1] stays 0.
//   fps_finish_kernel   ids and dist_sq out of best[], the count, cover_sq, the padding tails; owners by id.
// Nothing waits on another workgroup; every loop's trip count is known at launch; nothing is read back by the device
// form.  Which tiles are touched depends on the order of the points, the result does not.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

#include "fps_plan.h"
#include "fps_terms.h"
#include "knn_grid.h"
#include "range_walk.h"

namespace pcgx {

constexpr int kFpsTile = 256;   // points of a tile
constexpr int kFpsBlock = 256;  // threads of every kernel here: four waves
constexpr int kFpsWaves = kFpsBlock / 64;
constexpr int kFpsPerLane = kFpsTile / 64;
static_assert(FpsFacts().tile == kFpsTile && FpsFacts().waves == kFpsWaves && FpsFacts().wave == 64,
              "fps_plan.h plans with these");

__global__ __launch_bounds__(kFpsBlock) void fps_gather_kernel(TreeView tv, int64_t n, float *__restrict__ xyz) {
  const uint32_t b = blockIdx.x * (uint32_t)kFpsBlock + threadIdx.x;
  if (b < 1u || b >= (1u << tv.depth)) return;
  const uint32_t size = node_size(b, 31 - __clz((int)b), (uint32_t)tv.n + 1u);
  if (size < 1u || size > (uint32_t)tv.n) return;  // no such node
  const float4 nd = node_at(tv.nodes, b);
  const uint32_t id = __float_as_uint(nd.w);
  if ((int64_t)id >= n) return;
  xyz[3 * (size_t)id] = nd.x;
  xyz[3 * (size_t)id + 1] = nd.y;
  xyz[3 * (size_t)id + 2] = nd.z;
}

// the largest of the wave's keys, in every lane
__device__ __forceinline__ uint64_t fps_wave_max(uint64_t k) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t hi = __shfl_xor((uint32_t)(k >> 32), o), lo = __shfl_xor((uint32_t)k, o);
    const uint64_t other = ((uint64_t)hi << 32) | lo;
    k = other > k ? other : k;
  }
  return k;
}

// best = max(best, key) where that changes anything (most workgroups' keys are not the largest: a plain load first)
__device__ __forceinline__ void fps_offer(unsigned long long *best, const uint64_t key) {
  if (key == 0ull) return;
  if (__hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= key) return;
  atomicMax(best, (unsigned long long)key);
}

struct FpsState {
  const float *xyz;     // [3 n] by id
  float4 *rec;          // by position
  float *d;
  int32_t *owner;       // the owning pick's position in the pick order
  uint8_t *cand;
  uint32_t *pos_of;     // by id
  float4 *box;          // [2 tiles]
  unsigned long long *key;   // [tiles]
  unsigned long long *best;  // [picks + 1]
  uint32_t *touched;         // [picks] or nullptr: the tiles step j touched (measurements: pcgx_kdtree_fps_prep_dev)
  int64_t n, tiles;
};

__global__ __launch_bounds__(kFpsBlock) void fps_prep_kernel(FpsState S, const int32_t *__restrict__ perm, int64_t start) {
  __shared__ unsigned long long s_key[kFpsWaves];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
  const int64_t tile = (int64_t)blockIdx.x * kFpsWaves + wave;
  const float inf = __builtin_inff();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  uint64_t key = 0ull;
  if (tile < S.tiles) {
    for (int q = 0; q < kFpsPerLane; q++) {
      const int64_t pos = tile * kFpsTile + q * 64 + lane;
      if (pos >= S.n) continue;
      const uint32_t id = (uint32_t)perm[pos];
      const float x = S.xyz[3 * (size_t)id], y = S.xyz[3 * (size_t)id + 1], z = S.xyz[3 * (size_t)id + 2];
      const bool el = fps_eligible(x, y, z);
      S.rec[pos] = make_float4(x, y, z, __uint_as_float(id));
      S.d[pos] = inf;
      S.owner[pos] = -1;
      S.cand[pos] = el ? (uint8_t)1 : (uint8_t)0;
      S.pos_of[id] = (uint32_t)pos;
      if (!el) continue;
      lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
      hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
      const uint64_t k = fps_key(inf, id);
      key = k > key ? k : key;
    }
    for (int o = 32; o > 0; o >>= 1)
      for (int k = 0; k < 3; k++) {
        lo[k] = fminf(lo[k], __shfl_xor(lo[k], o));
        hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o));
      }
    key = fps_wave_max(key);
    if (lane == 0) {
      S.box[2 * tile] = make_float4(lo[0], lo[1], lo[2], 0.0f);
      S.box[2 * tile + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
      S.key[tile] = key;
    }
  }
  // the first pick: the caller's (checked on the host), else the smallest eligible id -- the largest key at d = +inf
  if (start >= 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) S.best[0] = fps_key(inf, (uint32_t)start);
    return;
  }
  if (lane == 0) s_key[wave] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t m = 0ull;
    for (int w = 0; w < kFpsWaves; w++) m = s_key[w] > m ? s_key[w] : m;
    fps_offer(S.best, m);
  }
}

// One touched tile, the whole wave's: the key of its candidates after pick j at s (id sid).
__device__ __forceinline__ uint64_t fps_touch(const FpsState &S, const int64_t tile, const int lane, const float sx,
                                              const float sy, const float sz, const uint32_t sid, const int32_t j) {
  uint64_t key = 0ull;
  for (int q = 0; q < kFpsPerLane; q++) {
    const int64_t pos = tile * kFpsTile + q * 64 + lane;
    if (pos >= S.n || S.cand[pos] == 0) continue;
    const float4 r = S.rec[pos];
    float d = S.d[pos];
    const float nd = ref_dist_sq(r.x, r.y, r.z, sx, sy, sz);
    if (fps_updates(nd, d)) {
      d = nd;
      S.d[pos] = nd;
      S.owner[pos] = j;
    }
    const uint32_t id = __float_as_uint(r.w);
    if (id == sid) {
      S.cand[pos] = 0;  // picked: never a candidate again
      continue;
    }
    const uint64_t k = fps_key(d, id);
    key = k > key ? k : key;
  }
  key = fps_wave_max(key);
  if (lane == 0) S.key[tile] = key;
  return key;
}

// wg_tiles: tiles of a workgroup, a multiple of kFpsWaves; a wave takes wg_tiles / kFpsWaves consecutive ones.
__global__ __launch_bounds__(kFpsBlock) void fps_pick_kernel(FpsState S, int32_t j, int32_t wg_tiles) {
  __shared__ unsigned long long s_key[kFpsWaves];
  const uint64_t pick = S.best[j];
  if (pick == 0ull) return;  // nothing left: best[j + 1] stays 0
  const uint32_t sid = fps_key_id(pick);
  const float sx = S.xyz[3 * (size_t)sid], sy = S.xyz[3 * (size_t)sid + 1], sz = S.xyz[3 * (size_t)sid + 2];
  const int64_t stile = (int64_t)(S.pos_of[sid] / (uint32_t)kFpsTile);
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
  const int per_wave = wg_tiles / kFpsWaves;
  const int64_t wbase = (int64_t)blockIdx.x * wg_tiles + (int64_t)wave * per_wave;
  // a lane a tile (per_wave <= 64, the plan's): its key, and whether the pick can lower anything in it
  const int64_t mine = wbase + lane;
  uint64_t best = 0ull;
  bool touch = false;
  if (lane < per_wave && mine < S.tiles) {
    best = S.key[mine];
    const float4 lo = S.box[2 * mine], hi = S.box[2 * mine + 1];
    const float lower = fps_box_lower(sx, sy, sz, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
    touch = !fps_skips(lower, fps_key_d(best)) || mine == stile;  // (the pick's own tile: it leaves the candidates)
  }
  unsigned long long todo = __ballot(touch);
  if (S.touched && lane == 0 && todo != 0ull) atomicAdd(S.touched + j, (uint32_t)__popcll(todo));
  while (todo != 0ull) {  // uniform: at most per_wave trips
    const int b = __builtin_ctzll(todo);
    todo &= todo - 1ull;
    const uint64_t k = fps_touch(S, wbase + b, lane, sx, sy, sz, sid, j);
    if (lane == b) best = k;
  }
  best = fps_wave_max(best);
  if (lane == 0) s_key[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t m = 0ull;
    for (int w = 0; w < kFpsWaves; w++) m = s_key[w] > m ? s_key[w] : m;
    fps_offer(S.best + j + 1, m);
  }
}

// best == nullptr (no pick was possible: Len() == 0, count == 0): every slot its padding value.
__global__ __launch_bounds__(kFpsBlock) void fps_finish_kernel(const unsigned long long *__restrict__ best, int64_t picks,
                                                               int64_t count, const float4 *__restrict__ rec,
                                                               const int32_t *__restrict__ owner_pos, int64_t n,
                                                               int32_t *__restrict__ ids, int32_t *__restrict__ n_ids,
                                                               float *__restrict__ dist_sq, float *__restrict__ cover_sq,
                                                               int32_t *__restrict__ owner) {
  const int64_t i = (int64_t)blockIdx.x * kFpsBlock + threadIdx.x;
  if (i < count) {
    const uint64_t k = best && i < picks ? best[i] : 0ull;
    if (ids) ids[i] = k ? (int32_t)fps_key_id(k) : kFpsNoId;
    if (dist_sq) dist_sq[i] = k ? fps_key_d(k) : kFpsNoDist;
    // the picks are a run of nonzero words: its last member knows the count
    if (n_ids && k && (i + 1 == picks || best[i + 1] == 0ull)) *n_ids = (int32_t)(i + 1);
  }
  if (i == 0) {
    const uint64_t first = best && picks > 0 ? best[0] : 0ull, next = best ? best[picks] : 0ull;
    if (n_ids && first == 0ull) *n_ids = 0;
    if (cover_sq) *cover_sq = first && next ? fps_key_d(next) : kFpsNoDist;
  }
  if (owner && i < n) {
    if (!rec) {
      owner[i] = kFpsNoId;
    } else {
      const int32_t p = owner_pos[i];
      owner[__float_as_uint(rec[i].w)] = p >= 0 ? (int32_t)fps_key_id(best[p]) : kFpsNoId;
    }
  }
}

static pcgx_status fps_finish(const unsigned long long *best, int64_t picks, int64_t count, const float4 *rec,
                              const int32_t *owner_pos, int64_t n, int32_t *d_ids, int32_t *d_n_ids, float *d_dist_sq,
                              float *d_cover_sq, int32_t *d_owner, hipStream_t st) {
  const int64_t items = count > n ? count : n;
  const unsigned blocks = (unsigned)((items > 0 ? items : 1) + kFpsBlock - 1) / kFpsBlock;
  hipLaunchKernelGGL(fps_finish_kernel, dim3(blocks), dim3(kFpsBlock), 0, st, best, picks, count, rec, owner_pos, n, d_ids,
                     d_n_ids, d_dist_sq, d_cover_sq, d_owner);
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

// The box the Morton keys are taken over: the base cloud's where it is finite, else that of its finite points.
static void fps_order_box(const pcgx_kdtree *t, float lo[3], float hi[3]) {
  bool ok = true;
  for (int k = 0; k < 3; k++) {
    lo[k] = t->bbox_lo[k];
    hi[k] = t->bbox_hi[k];
    ok = ok && fps_finite(lo[k]) && fps_finite(hi[k]);
  }
  if (ok) return;
  bool any = false;
  const float *pp = t->points.data();
  for (int64_t i = 0; i < t->n; i++) {
    const float *p = pp + 3 * i;
    if (!fps_eligible(p[0], p[1], p[2])) continue;
    for (int k = 0; k < 3; k++) {
      lo[k] = !any || p[k] < lo[k] ? p[k] : lo[k];
      hi[k] = !any || p[k] > hi[k] ? p[k] : hi[k];
    }
    any = true;
  }
  if (!any)
    for (int k = 0; k < 3; k++) lo[k] = hi[k] = 0.0f;
}

struct FpsPrepared {
  FpsState S;
  FpsPlan plan;
};

// Len() > 0, count > 0, start checked: the ordered copy, the tiles and best[0].  Temporaries from ctx().arena, which
// the caller has begun.
static pcgx_status fps_prepare(const pcgx_kdtree *t, int64_t count, int64_t start, uint32_t *d_touched, FpsPrepared *out,
                               hipStream_t st) {
  Arena &ar = ctx().arena;
  const int64_t n = t->n;
  const FpsPlan p = plan_fps(n, count);
  FpsState S{};
  S.touched = d_touched;
  S.n = n;
  S.tiles = p.tiles;
  void *buf[kFpsBufs] = {};
  for (int b = 0; b < kFpsBufs; b++) PCGX_TRY(ar.alloc(p.bytes[b], &buf[b]));
  float *xyz = (float *)buf[kFpsBufXyz];
  int32_t *perm = (int32_t *)buf[kFpsBufPerm];
  S.xyz = xyz;
  S.rec = (float4 *)buf[kFpsBufRec];
  S.d = (float *)buf[kFpsBufDist];
  S.owner = (int32_t *)buf[kFpsBufOwner];
  S.cand = (uint8_t *)buf[kFpsBufCand];
  S.pos_of = (uint32_t *)buf[kFpsBufPos];
  S.box = (float4 *)buf[kFpsBufBox];
  S.key = (unsigned long long *)buf[kFpsBufKey];
  S.best = (unsigned long long *)buf[kFpsBufBest];
  const pcgx_kdtree *a = nullptr;
  bool empty = false;
  PCGX_TRY(resolve_tree(t, &a, &empty));  // after DeletePoint: the tree over the remaining points, original ids
  PCGX_HIP_TRY(hipMemsetAsync(xyz, 0xff, p.bytes[kFpsBufXyz], st));  // NaN: an id the tree does not hold
  PCGX_HIP_TRY(hipMemsetAsync(S.best, 0, p.bytes[kFpsBufBest], st));
  if (!empty) {
    const TreeView tv = a->view();
    const unsigned slots = 1u << tv.depth;
    hipLaunchKernelGGL(fps_gather_kernel, dim3((slots + kFpsBlock - 1u) / kFpsBlock), dim3(kFpsBlock), 0, st, tv, n, xyz);
    PCGX_HIP_TRY(hipGetLastError());
  }
  float lo[3], hi[3];
  fps_order_box(t, lo, hi);
  PCGX_TRY(morton_order(xyz, n, lo, hi, perm, st));
  hipLaunchKernelGGL(fps_prep_kernel, dim3((unsigned)((p.tiles + kFpsWaves - 1) / kFpsWaves)), dim3(kFpsBlock), 0, st, S,
                     (const int32_t *)perm, start);
  PCGX_HIP_TRY(hipGetLastError());
  out->S = S;
  out->plan = p;
  return PCGX_OK;
}

// A launch per step.
static pcgx_status fps_picks_enqueue(const FpsPrepared &f, hipStream_t st) {
  const FpsPlan &p = f.plan;
  for (int64_t j = 0; j < p.picks; j++) {
    hipLaunchKernelGGL(fps_pick_kernel, dim3((unsigned)p.workgroups), dim3(kFpsBlock), 0, st, f.S, (int32_t)j, p.wg_tiles);
    if ((j & 63) == 63) PCGX_HIP_TRY(hipGetLastError());  // (a count may be millions: no enqueueing behind a failure)
  }
  PCGX_HIP_TRY(hipGetLastError());
  return PCGX_OK;
}

}  // namespace pcgx

using namespace pcgx;

namespace {

constexpr int64_t kFpsMaxCount = 0x7fffffff;  // pick positions are int32 on the device

// is id `start` in E?  The host knows the deletions and has the points' copy.
bool fps_start_ok(const pcgx_kdtree *t, int64_t start) {
  if (t->n_deleted > 0 && t->deleted[(size_t)start]) return false;
  const float *p = t->points.data() + 3 * start;
  return fps_eligible(p[0], p[1], p[2]);
}

pcgx_status fps_check(const char *fn, const pcgx_kdtree *t, int64_t count, int64_t start, const void *ids,
                      const void *n_ids) {
  if (!t) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (count < 0 || count > kFpsMaxCount) return fail(PCGX_E_INVALID, "%s: count must be in [0, 2^31 - 1]", fn);
  if (t->n > kFpsMaxCount) return fail(PCGX_E_INVALID, "%s: more than 2^31 - 1 points", fn);  // ids are int32 on the device
  if (t->n > 0 && count > 0 && (!ids || !n_ids)) return fail(PCGX_E_INVALID, "%s: NULL ids or n_ids", fn);
  if (start < -1 || (start >= 0 && start >= t->n))
    return fail(PCGX_E_INVALID, "%s: start must be -1 or a point id below Len()", fn);
  if (start >= 0 && !fps_start_ok(t, start))
    return fail(PCGX_E_INVALID, "%s: start is a deleted point or has a non-finite coordinate", fn);
  return PCGX_OK;
}

struct FpsTreeFree {
  void operator()(pcgx_kdtree *t) const { pcgx_kdtree_free(t); }
};

__global__ __launch_bounds__(256) void fps_filter_xyz_kernel(const uint8_t *__restrict__ data, int64_t n, int32_t stride,
                                                             int32_t off, float *__restrict__ xyz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t *p = data + i * stride + off;
  for (int k = 0; k < 3; k++) {
    uint32_t w = 0u;  // (records need not be aligned)
    for (int b = 0; b < 4; b++) w |= (uint32_t)p[4 * k + b] << (8 * b);
    xyz[3 * i + k] = __uint_as_float(w);
  }
}

// out record j = the record of pick j: orig[ids[j]] is its index in the cloud
__global__ __launch_bounds__(256) void fps_filter_copy_kernel(const uint8_t *__restrict__ data, int32_t stride,
                                                              const int32_t *__restrict__ ids,
                                                              const int32_t *__restrict__ n_ids,
                                                              const int64_t *__restrict__ orig, uint8_t *__restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= (int64_t)*n_ids) return;
  const uint8_t *src = data + orig[ids[j]] * stride;
  uint8_t *dst = out + j * stride;
  for (int32_t b = 0; b < stride; b++) dst[b] = src[b];
}

pcgx_status fps_filter_check(const char *fn, const void *data, int64_t n, int32_t stride, int32_t off, int64_t count,
                             int64_t start, const void *out, const int64_t *out_n) {
  if (!out_n || n < 0 || (n > 0 && (!data || !out))) return fail(PCGX_E_INVALID, "%s: bad argument", fn);
  if (count < 0 || count > kFpsMaxCount) return fail(PCGX_E_INVALID, "%s: count must be in [0, 2^31 - 1]", fn);
  if (start < -1) return fail(PCGX_E_INVALID, "%s: start must be -1 or an index among the finite records", fn);
  if (stride < 12 || off < 0 || off + 12 > stride)
    return fail(PCGX_E_BAD_FIELD, "%s: stride %d / xyz offset %d do not hold an xyz triple", fn, (int)stride, (int)off);
  if (n == 0) return fail(PCGX_E_NO_POINT, "%s: empty cloud", fn);
  return PCGX_OK;
}

// The whole filter on device records; temporaries from `ka` (begun by the caller).  Returns with st drained.
pcgx_status fps_filter_run(const char *fn, const uint8_t *d_data, int64_t n, int32_t stride, int32_t off, int64_t count,
                           int64_t start, uint8_t *d_out, int64_t *out_n, hipStream_t st, Arena &ka) {
  float *d_xyz = nullptr;
  PCGX_TRY(ka.alloc_n((size_t)n * 3, &d_xyz));
  hipLaunchKernelGGL(fps_filter_xyz_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_data, n, stride, off,
                     d_xyz);
  PCGX_HIP_TRY(hipGetLastError());
  RawVector<float> h_xyz((size_t)n * 3);
  PCGX_TRY(staged_download(h_xyz.data(), d_xyz, (size_t)n * 12, st));
  // the finite records, in input order (the tree build wants them on the host anyway)
  RawVector<int64_t> orig((size_t)n);
  int64_t m = 0;
  for (int64_t i = 0; i < n; i++) {
    const float *p = h_xyz.data() + 3 * i;
    if (!fps_eligible(p[0], p[1], p[2])) continue;
    if (m != i) memcpy(h_xyz.data() + 3 * m, p, 12);
    orig[(size_t)m++] = i;
  }
  if (m == 0) return fail(PCGX_E_NO_POINT, "%s: no finite point", fn);
  if (start >= m) return fail(PCGX_E_INVALID, "%s: start must be -1 or an index among the %lld finite records", fn, (long long)m);
  const int64_t c = count < m ? count : m;
  if (c == 0) {
    *out_n = 0;
    return PCGX_OK;
  }
  pcgx_kdtree *raw = nullptr;
  PCGX_TRY(pcgx_kdtree_build(h_xyz.data(), m, 12, 0, &raw));
  std::unique_ptr<pcgx_kdtree, FpsTreeFree> tree(raw);
  int32_t *d_ids = nullptr;  // [c], the count
  int64_t *d_orig = nullptr;
  PCGX_TRY(ka.alloc_n((size_t)c + 1, &d_ids));
  PCGX_TRY(ka.alloc_n((size_t)m, &d_orig));
  PCGX_TRY(staged_upload(d_orig, orig.data(), (size_t)m * 8, st));
  PCGX_TRY(pcgx_kdtree_fps_dev(tree.get(), c, start, d_ids, d_ids + c, nullptr, nullptr, nullptr, st));
  hipLaunchKernelGGL(fps_filter_copy_kernel, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, st, d_data, stride,
                     (const int32_t *)d_ids, (const int32_t *)(d_ids + c), (const int64_t *)d_orig, d_out);
  PCGX_HIP_TRY(hipGetLastError());
  int32_t got = 0;
  PCGX_HIP_TRY(hipMemcpyAsync(&got, d_ids + c, 4, hipMemcpyDeviceToHost, st));
  PCGX_HIP_TRY(hipStreamSynchronize(st));  // (the tree is freed below: its kernels must be done)
  *out_n = got;
  return PCGX_OK;
}

}  // namespace

extern "C" pcgx_status pcgx_kdtree_fps_dev(const pcgx_kdtree *t, int64_t count, int64_t start, int32_t *d_ids,
                                           int32_t *d_n_ids, float *d_dist_sq, float *d_cover_sq, int32_t *d_owner,
                                           void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(fps_check("pcgx_kdtree_fps_dev", t, count, start, d_ids, d_n_ids));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  const int64_t n = t->n;
  if (n == 0 || count == 0)
    return fps_finish(nullptr, 0, count, nullptr, nullptr, n, d_ids, d_n_ids, d_dist_sq, d_cover_sq, d_owner, st);
  PCGX_TRY(ctx().arena.begin(st));
  FpsPrepared f;
  PCGX_TRY(fps_prepare(t, count, start, nullptr, &f, st));
  PCGX_TRY(fps_picks_enqueue(f, st));
  return fps_finish(f.S.best, f.plan.picks, count, f.S.rec, f.S.owner, n, d_ids, d_n_ids, d_dist_sq, d_cover_sq, d_owner, st);
}

// The plan of a call, for the tests' sizes: out4 = {points per tile, tiles, tiles per pick workgroup, pick workgroups}.
extern "C" pcgx_status pcgx_fps_plan(int64_t n, int64_t count, int64_t out4[4]) {
  if (!out4 || n < 0 || count < 0) return fail(PCGX_E_INVALID, "pcgx_fps_plan: bad argument");
  const FpsPlan p = plan_fps(n, count);
  out4[0] = p.tile;
  out4[1] = p.tiles;
  out4[2] = p.wg_tiles;
  out4[3] = p.workgroups;
  return PCGX_OK;
}

// Measurements (tools/fps_probe.py).  d_touched == NULL: the prep stage alone, whose cost the probe reports beside the
// whole call's.  Else the steps run too, no output but d_touched[j] = the tiles step j touched (uint32 [min(count, Len())]).
extern "C" pcgx_status pcgx_kdtree_fps_prep_dev(const pcgx_kdtree *t, int64_t count, uint32_t *d_touched, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(fps_check("pcgx_kdtree_fps_prep_dev", t, count, -1, t, t));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  if (t->n == 0 || count == 0) return PCGX_OK;
  PCGX_TRY(ctx().arena.begin(st));
  FpsPrepared f;
  if (d_touched) PCGX_HIP_TRY(hipMemsetAsync(d_touched, 0, (size_t)(count < t->n ? count : t->n) * 4, st));
  PCGX_TRY(fps_prepare(t, count, -1, d_touched, &f, st));
  return d_touched ? fps_picks_enqueue(f, st) : PCGX_OK;
}

extern "C" pcgx_status pcgx_kdtree_fps(const pcgx_kdtree *t, int64_t count, int64_t start, int64_t *ids, int64_t *n_ids,
                                       float *dist_sq, float *cover_sq, int64_t *owner) {
  PCGX_API_CALL();
  PCGX_TRY(fps_check("pcgx_kdtree_fps", t, count, start, ids, n_ids));
  const int64_t n = t->n;
  if (n == 0 || count == 0) {  // every slot its padding value
    if (n_ids) *n_ids = 0;
    for (int64_t j = 0; j < count; j++) {
      if (ids) ids[j] = kFpsNoId;
      if (dist_sq) dist_sq[j] = kFpsNoDist;
    }
    if (cover_sq) *cover_sq = kFpsNoDist;
    if (owner)
      for (int64_t i = 0; i < n; i++) owner[i] = kFpsNoId;
    return PCGX_OK;
  }
  PCGX_TRY(ensure_init());
  // always on the device: the picks are the kernels', not a host restatement
  hipStream_t st = ctx().stream;
  Arena &ha = ctx().host_arena;
  PCGX_TRY(ha.begin(st));
  const size_t c = (size_t)count;
  int32_t *d_out = nullptr, *d_owner = nullptr;  // ids [count], the count, cover_sq; owner [n]
  float *d_dist = nullptr;
  PCGX_TRY(ha.alloc_n(c + 2, &d_out));
  PCGX_TRY(ha.alloc_n(c, &d_dist));
  if (owner) PCGX_TRY(ha.alloc_n((size_t)n, &d_owner));
  PCGX_TRY(pcgx_kdtree_fps_dev(t, count, start, d_out, d_out + c, d_dist, (float *)(d_out + c + 1), d_owner, st));
  RawVector<int32_t> h(c + 2);
  PCGX_TRY(staged_download(h.data(), d_out, (c + 2) * 4, st));
  for (size_t j = 0; j < c; j++) ids[j] = h[j];
  *n_ids = h[c];
  if (cover_sq) memcpy(cover_sq, &h[c + 1], 4);
  if (dist_sq) PCGX_TRY(staged_download(dist_sq, d_dist, c * 4, st));
  if (owner) {
    RawVector<int32_t> ho((size_t)n);
    PCGX_TRY(staged_download(ho.data(), d_owner, (size_t)n * 4, st));
    for (int64_t i = 0; i < n; i++) owner[i] = ho[(size_t)i];
  }
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_fps_filter_dev(const void *d_data, int64_t n, int32_t stride, int32_t xyz_off, int64_t count,
                                           int64_t start, void *d_out, int64_t *out_n, void *stream) {
  PCGX_API_LOCK();
  PCGX_TRY(fps_filter_check("pcgx_fps_filter_dev", d_data, n, stride, xyz_off, count, start, d_out, out_n));
  PCGX_TRY(ensure_init());
  hipStream_t st = pick_stream(stream);
  Arena &ka = ctx().host_arena;
  PCGX_TRY(ka.begin(st));
  return fps_filter_run("pcgx_fps_filter_dev", (const uint8_t *)d_data, n, stride, xyz_off, count, start, (uint8_t *)d_out,
                        out_n, st, ka);
}

extern "C" pcgx_status pcgx_fps_filter(const void *data, int64_t n, int32_t stride, int32_t xyz_off, int64_t count,
                                       int64_t start, void *out_data, int64_t *out_n) {
  PCGX_API_CALL();
  PCGX_TRY(fps_filter_check("pcgx_fps_filter", data, n, stride, xyz_off, count, start, out_data, out_n));
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ka = ctx().host_arena;
  PCGX_TRY(ka.begin(st));
  const size_t bytes = (size_t)n * (size_t)stride;
  uint8_t *d_in = nullptr, *d_out = nullptr;
  PCGX_TRY(ka.alloc_n(bytes, &d_in));
  PCGX_TRY(ka.alloc_n(bytes, &d_out));
  PCGX_TRY(staged_upload(d_in, data, bytes, st));
  int64_t kept = 0;
  PCGX_TRY(fps_filter_run("pcgx_fps_filter", d_in, n, stride, xyz_off, count, start, d_out, &kept, st, ka));
  if (kept > 0) PCGX_TRY(staged_download(out_data, d_out, (size_t)kept * (size_t)stride, st));
  *out_n = kept;
  return PCGX_OK;
}
