// sac.hip -- sample consensus plane detection over the bucket voxel grid on gfx950.
//
// Reference:
//   pc/sac/sac.go:33-59           SAC.Compute(n): draw 3 ids, Fit, Evaluate, keep the first strictly best
//   pc/sac/surface.go:36-181      voxelGridSurfaceModel.Fit: the plane through three points, cut by the grid's box
//   pc/sac/surface.go:202-220     Evaluate: a float32 lattice over the cut, sum of the bucket lengths of the
//                                 distinct voxels it hits
//   pc/sac/surface.go:222-240     Inliers(d) / IsIn(p, d)
//
// Neither Fit nor Evaluate draws random numbers, so the caller's sampler draws all 3n ids first (in the
// reference's order) and one call evaluates every hypothesis:
//   sac_fit_kernel       one lane per hypothesis: ok flag, coefficients, lattice extents (na, nb)
//   sac_evaluate_kernel  one 1024-lane workgroup per ok hypothesis, handed out through a work counter (lattice
//                        sizes differ by orders of magnitude); the a and b sequences are the reference's float32
//                        accumulators, computed serially into LDS, the lattice is spread over the workgroup.
//                        A voxel counts once: one bit per OCCUPIED voxel (empty ones add 0), in LDS when the grid
//                        has at most kLdsBitmapCells of them, else in a global slot the workgroup owns and clears
//                        after each hypothesis.  First-max argmax: one 64-bit atomicMax on (score, ~index).
//   sac_inliers_*        Inliers(d): an order-preserving compaction over the cloud (bucket_grid.h's tile scan)
// All arithmetic is float32 left to right without contraction (build.py: -ffp-contract=off), Norm is
// float32(sqrt(float64(NormSq))) (mat/vec3.go:22-28), divides are correctly rounded.
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "bucket_grid.h"

namespace pcgx {

// Longest a or b sequence of one hypothesis (its serial float32 accumulation lives in LDS); a longer one is
// PCGX_E_TOO_LARGE, never a shorter lattice.
constexpr int kSacSeqCap = 8192;
// Occupied voxels whose "counted" bits fit the workgroup's LDS next to the two sequences (64 KiB): 80 KiB of bits.
constexpr int64_t kLdsBitmapCells = 20480 * 32;
constexpr int kSacEvalBlock = 1024;

// ---- surface.go:108-135: the 36 listed edge candidates in their order, vertex v = axis * 4 + index
struct EdgeTables {
  int a[36], b[36];             // ends
  int slot_a[36], slot_b[36];   // the edge's position in edge[a] / edge[b] when every candidate is appended
  int partner[12][6];           // partner[v][s]: the other end of v's s-th candidate
  int count[12];
};
constexpr int kEdgeList[36][4] = {
    {0, 0, 1, 0}, {0, 0, 1, 2}, {0, 0, 2, 0}, {0, 0, 2, 2}, {0, 1, 1, 1}, {0, 1, 1, 3}, {0, 1, 2, 0}, {0, 1, 2, 2},
    {0, 2, 1, 0}, {0, 2, 1, 2}, {0, 2, 2, 1}, {0, 2, 2, 3}, {0, 3, 1, 1}, {0, 3, 1, 3}, {0, 3, 2, 1}, {0, 3, 2, 3},
    {1, 0, 2, 0}, {1, 0, 2, 1}, {1, 1, 2, 0}, {1, 1, 2, 1}, {1, 2, 2, 2}, {1, 2, 2, 3}, {1, 3, 2, 2}, {1, 3, 2, 3},
    {0, 0, 0, 2}, {0, 0, 0, 1}, {0, 1, 0, 3}, {0, 3, 0, 2}, {1, 0, 1, 2}, {1, 0, 1, 1}, {1, 1, 1, 3}, {1, 3, 1, 2},
    {2, 0, 2, 2}, {2, 0, 2, 1}, {2, 1, 2, 3}, {2, 3, 2, 2}};
constexpr EdgeTables make_edge_tables() {
  EdgeTables t{};
  for (int p = 0; p < 36; p++) {
    const int a = kEdgeList[p][0] * 4 + kEdgeList[p][1], b = kEdgeList[p][2] * 4 + kEdgeList[p][3];
    t.a[p] = a;
    t.b[p] = b;
    t.slot_a[p] = t.count[a];
    t.partner[a][t.count[a]++] = b;
    t.slot_b[p] = t.count[b];
    t.partner[b][t.count[b]++] = a;
  }
  return t;
}
constexpr EdgeTables kEdges = make_edge_tables();
static_assert(kEdges.count[0] == 6 && kEdges.count[11] == 6, "every crossing point has six candidate edges");

// every index below is a template argument: o[][] and the edge masks stay in registers
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

__device__ __forceinline__ bool near_zero(float a) { return -0.01f < a && a < 0.01f; }   // surface.go:183-185
__device__ __forceinline__ bool near_zero_sq(float a) { return a < 0.0001f; }            // :187-189 (epsilon*epsilon, once)
__device__ __forceinline__ float dist_sq(const float a[3], const float b[3]) {
  return norm_sq3(a[0] - b[0], a[1] - b[1], a[2] - b[2]);
}
__device__ __forceinline__ float norm_f32(float sq) { return (float)__builtin_sqrt((double)sq); }

struct SacFitArgs {
  const float4 *xyz;
  const uint32_t *ids;  // [3n]
  int64_t n;
  float vg_min[3], vg_size[3];
  float resolution;
  int32_t *ok;
  pcgx_sac_plane *coeff;
  uint32_t *ext;  // [2n]: na, nb
  int64_t *score;
  uint32_t *too_large;
};

// voxelGridSurfaceModel.Fit (surface.go:36-181) of one hypothesis
__global__ __launch_bounds__(256) void sac_fit_kernel(SacFitArgs A) {
  const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (h >= A.n) return;
  A.score[h] = 0;
  float p[3][3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float4 q = A.xyz[A.ids[3 * h + j]];
    p[j][0] = q.x - A.vg_min[0];
    p[j][1] = q.y - A.vg_min[1];
    p[j][2] = q.z - A.vg_min[2];
  }
  const float v1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
  const float v2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
  float nrm[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
  bool ok = !near_zero_sq(norm_sq3(nrm[0], nrm[1], nrm[2]));
  const float inv = 1.0f / norm_f32(norm_sq3(nrm[0], nrm[1], nrm[2]));  // Normalized: v.Mul(1 / Norm)
  nrm[0] = nrm[0] * inv;
  nrm[1] = nrm[1] * inv;
  nrm[2] = nrm[2] * inv;
  const float d = nrm[0] * p[0][0] + nrm[1] * p[0][1] + nrm[2] * p[0][2];
  const float *vs = A.vg_size;
  const bool valid[3] = {!near_zero(nrm[0]), !near_zero(nrm[1]), !near_zero(nrm[2])};
  const float vgn[3] = {nrm[0] * vs[0], nrm[1] * vs[1], nrm[2] * vs[2]};
  float o[12][3] = {};
  if (valid[0]) {
    o[0][0] = (d - vgn[1] - vgn[2]) / nrm[0]; o[0][1] = vs[1]; o[0][2] = vs[2];  // y+z+
    o[1][0] = (d - vgn[1]) / nrm[0];          o[1][1] = vs[1];                   // y+z-
    o[2][0] = (d - vgn[2]) / nrm[0];                           o[2][2] = vs[2];  // y-z+
    o[3][0] = d / nrm[0];                                                        // y-z-
  }
  if (valid[1]) {
    o[4][0] = vs[0]; o[4][1] = (d - vgn[0] - vgn[2]) / nrm[1]; o[4][2] = vs[2];  // x+z+
    o[5][0] = vs[0]; o[5][1] = (d - vgn[0]) / nrm[1];                            // x+z-
                     o[6][1] = (d - vgn[2]) / nrm[1];          o[6][2] = vs[2];  // x-z+
                     o[7][1] = d / nrm[1];                                       // x-z-
  }
  if (valid[2]) {
    o[8][0] = vs[0]; o[8][1] = vs[1]; o[8][2] = (d - vgn[0] - vgn[1]) / nrm[2];  // x+y+
    o[9][0] = vs[0];                  o[9][2] = (d - vgn[0]) / nrm[2];           // x+y-
                     o[10][1] = vs[1]; o[10][2] = (d - vgn[1]) / nrm[2];         // x-y+
                                       o[11][2] = d / nrm[2];                    // x-y-
  }
  bool inside[12];
#pragma unroll
  for (int v = 0; v < 12; v++)
    inside[v] = valid[v / 4] && !(o[v][0] < 0 || vs[0] < o[v][0] || o[v][1] < 0 || vs[1] < o[v][1] || o[v][2] < 0 ||
                                  vs[2] < o[v][2]);
  // edge[v] as a mask over v's candidates in append order
  uint32_t mask[12] = {};
  static_for<0, 36>([&](auto P) {
    constexpr int pp = decltype(P)::value;
    constexpr int a = kEdges.a[pp], b = kEdges.b[pp];
    if (inside[a] && inside[b] && !near_zero_sq(dist_sq(o[a], o[b]))) {
      mask[a] |= 1u << kEdges.slot_a[pp];
      mask[b] |= 1u << kEdges.slot_b[pp];
    }
  });
  // remove duplication (an entry goes when a later one is near it), then the vertex with exactly two edges and the
  // largest summed squared length, the first one on a tie
  float max_len_sq = 0.0f;
  float o0[3] = {}, o1[3] = {}, o2[3] = {};
  static_for<0, 12>([&](auto V) {
    constexpr int v = decltype(V)::value;
    uint32_t kept = 0;
    static_for<0, 6>([&](auto S) {
      constexpr int s = decltype(S)::value;
      bool keep = (mask[v] >> s) & 1u;
      static_for<s + 1, 6>([&](auto T) {
        constexpr int t = decltype(T)::value;
        if (((mask[v] >> t) & 1u) && near_zero_sq(dist_sq(o[kEdges.partner[v][s]], o[kEdges.partner[v][t]]))) keep = false;
      });
      kept |= (keep ? 1u : 0u) << s;
    });
    if (__builtin_popcount(kept) != 2) return;
    float e0[3] = {}, e1[3] = {}, l = 0.0f;
    int seen = 0;
    static_for<0, 6>([&](auto S) {
      constexpr int s = decltype(S)::value;
      constexpr int e = kEdges.partner[v][s];
      if ((kept >> s) & 1u) {
        l += dist_sq(o[v], o[e]);
        for (int k = 0; k < 3; k++) {
          if (seen == 0) e0[k] = o[e][k];
          else e1[k] = o[e][k];
        }
        seen++;
      }
    });
    if (l > max_len_sq) {
      max_len_sq = l;
      for (int k = 0; k < 3; k++) {
        o0[k] = e0[k];
        o1[k] = o[v][k];
        o2[k] = e1[k];
      }
    }
  });
  ok = ok && max_len_sq != 0.0f;  // (an ok == false Fit leaves the rest unused)
  const float ov1[3] = {o0[0] - o1[0], o0[1] - o1[1], o0[2] - o1[2]};
  const float ov2[3] = {o2[0] - o1[0], o2[1] - o1[1], o2[2] - o1[2]};
  const float r = A.resolution / 1.732050808f;  // sqrt3, converted to float32 once
  pcgx_sac_plane c;
  for (int k = 0; k < 3; k++) {
    c.origin[k] = o1[k] + A.vg_min[k];
    c.v1[k] = ov1[k];
    c.v2[k] = ov2[k];
    c.norm[k] = nrm[k];
  }
  c.l1 = r / norm_f32(norm_sq3(ov1[0], ov1[1], ov1[2]));
  c.l2 = r / norm_f32(norm_sq3(ov2[0], ov2[1], ov2[2]));
  c.d = d;
  if (!ok) memset(&c, 0, sizeof(c));
  // lattice extents: how many values the accumulators `a += l1` / `b += l2` take while <= 1 (surface.go:206-207)
  uint32_t na = 0, nb = 0;
  if (ok) {
    for (float a = 0.0f; a <= 1.0f && na <= (uint32_t)kSacSeqCap; a += c.l1) na++;
    for (float b = 0.0f; b <= 1.0f && nb <= (uint32_t)kSacSeqCap; b += c.l2) nb++;
    if (na > (uint32_t)kSacSeqCap || nb > (uint32_t)kSacSeqCap) atomicOr(A.too_large, 1u);
  }
  A.ok[h] = ok ? 1 : 0;
  A.coeff[h] = c;
  A.ext[2 * h] = na;
  A.ext[2 * h + 1] = nb;
}

struct SacEvalArgs {
  GridParams gp;
  const uint32_t *cell_addr;   // occupied voxels, ascending
  const uint32_t *cell_count;  // their bucket lengths
  int64_t m;
  const int32_t *ok;
  const pcgx_sac_plane *coeff;
  const uint32_t *ext;
  int64_t n;
  uint32_t *counter;             // next hypothesis (zero at launch)
  uint32_t *slots;               // global "counted" bits: slot_words per workgroup (zero at launch, kept zero)
  int64_t slot_words;
  int64_t *score;
  unsigned long long *best;      // (score << 32) | (0xffffffff - index), 0: none
};

// Evaluate (surface.go:202-220) of every ok hypothesis
template <bool kLdsBits>
__global__ __launch_bounds__(kSacEvalBlock) void sac_evaluate_kernel(SacEvalArgs A) {
  __shared__ float s_a[kSacSeqCap], s_b[kSacSeqCap];
  __shared__ uint32_t s_bits[kLdsBits ? kLdsBitmapCells / 32 : 1];
  __shared__ uint32_t s_sum[kSacEvalBlock / 64];
  __shared__ uint32_t s_h;
  uint32_t *bits = kLdsBits ? s_bits : A.slots + (int64_t)blockIdx.x * A.slot_words;
  const int words = (int)((A.m + 31) / 32);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (;;) {
    if (tid == 0) s_h = atomicAdd(A.counter, 1u);
    __syncthreads();
    const uint32_t h = s_h;
    if ((int64_t)h >= A.n) break;  // (uniform)
    const uint32_t na = A.ext[2 * h], nb = A.ext[2 * h + 1];
    // (a lattice too large for the sequences fails the whole call: pcgx_sac_plane_compute reads no score then)
    if (!A.ok[h] || na > (uint32_t)kSacSeqCap || nb > (uint32_t)kSacSeqCap) {
      __syncthreads();  // (s_h is read by every lane before lane 0 takes the next one)
      continue;
    }
    const pcgx_sac_plane c = A.coeff[h];
    if (tid == 0) {
      float a = 0.0f;
      for (uint32_t k = 0; k < na; k++, a += c.l1) s_a[k] = a;
    } else if (tid == 64) {
      float b = 0.0f;
      for (uint32_t k = 0; k < nb; k++, b += c.l2) s_b[k] = b;
    }
    if (kLdsBits)
      for (int w = tid; w < words; w += kSacEvalBlock) s_bits[w] = 0u;
    __syncthreads();
    // sample t = row * nb + col; each lane steps by kSacEvalBlock samples
    const uint32_t total = na * nb, qrow = kSacEvalBlock / nb, qcol = kSacEvalBlock % nb;
    uint32_t row = (uint32_t)tid / nb, col = (uint32_t)tid % nb, sum = 0;
    for (uint32_t t = tid; t < total; t += kSacEvalBlock) {
      const float a = s_a[row], b = s_b[col];
      const float px = (c.origin[0] + c.v1[0] * a) + c.v2[0] * b;
      const float py = (c.origin[1] + c.v1[1] * a) + c.v2[1] * b;
      const float pz = (c.origin[2] + c.v1[2] * a) + c.v2[2] * b;
      int64_t addr, xyz[3];
      if (grid_addr(A.gp, px, py, pz, &addr, xyz)) {
        const int64_t j = lower_bound_u32(A.cell_addr, A.m, (uint32_t)addr);
        if (j < A.m && A.cell_addr[j] == (uint32_t)addr) {
          const uint32_t bit = 1u << (j & 31);
          if (!(atomicOr(bits + (j >> 5), bit) & bit)) sum += A.cell_count[j];
        }
      }
      row += qrow;
      col += qcol;
      if (col >= nb) {
        col -= nb;
        row++;
      }
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
    if (lane == 0) s_sum[wave] = sum;
    if (!kLdsBits) __threadfence();
    __syncthreads();
    if (tid == 0) {
      uint32_t s = 0;
      for (int w = 0; w < kSacEvalBlock / 64; w++) s += s_sum[w];
      A.score[h] = s;
      if (s > 0) atomicMax(A.best, ((unsigned long long)s << 32) | (unsigned long long)(0xffffffffu - h));
    }
    if (!kLdsBits) {
      for (int w = tid; w < words; w += kSacEvalBlock) bits[w] = 0u;
      __threadfence();
    }
    __syncthreads();
  }
}

// Inliers(d) (surface.go:222-235): -d < norm . (p - vgMin) - d_plane < d
struct SacInlierArgs {
  const float4 *xyz;
  int64_t n;
  float vg_min[3], norm[3], dp, d;
};
__device__ __forceinline__ bool sac_is_in(const SacInlierArgs &A, int64_t j) {
  const float4 p = A.xyz[j];
  const float q0 = p.x - A.vg_min[0], q1 = p.y - A.vg_min[1], q2 = p.z - A.vg_min[2];
  const float dd = (A.norm[0] * q0 + A.norm[1] * q1 + A.norm[2] * q2) - A.dp;
  return -A.d < dd && dd < A.d;
}
__global__ __launch_bounds__(256) void sac_inliers_count_kernel(SacInlierArgs A, uint32_t *__restrict__ tile_count) {
  tile_flag_count(A.n, [&](int64_t j) { return sac_is_in(A, j); }, tile_count);
}
__global__ __launch_bounds__(1024) void sac_inliers_scan_kernel(uint32_t *__restrict__ tile_count, int ntiles,
                                                                uint32_t *__restrict__ total) {
  tile_scan(tile_count, ntiles, total);
}
__global__ __launch_bounds__(256) void sac_inliers_write_kernel(SacInlierArgs A, const uint32_t *__restrict__ tile_offset,
                                                                int64_t *__restrict__ out) {
  tile_flag_write(A.n, [&](int64_t j) { return sac_is_in(A, j); }, tile_offset,
                  [=](uint32_t slot, int64_t j) { out[slot] = j; });
}

// the model's copy of the cloud: xyz of every record, packed (w unused)
__global__ __launch_bounds__(256) void sac_pack_kernel(const uint8_t *__restrict__ data, int64_t n, int32_t stride,
                                                       int32_t off, float4 *__restrict__ xyz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v[3];
  __builtin_memcpy(v, data + i * stride + off, 12);
  xyz[i] = make_float4(v[0], v[1], v[2], 0.0f);
}

}  // namespace pcgx

using namespace pcgx;

struct pcgx_sac_plane_model {
  int64_t n = 0;                 // points of the model's cloud (ra.Len())
  float4 *d_xyz = nullptr;       // their xyz (library-owned)
  int64_t m = 0;                 // occupied voxels of the grid
  uint32_t *d_cell_addr = nullptr, *d_cell_count = nullptr;
  GridParams gp;
  float resolution = 0.0f;
  float vg_min[3], vg_size[3];   // surface.go:20-30
};

static void model_release(pcgx_sac_plane_model *m) {
  if (!m) return;
  dev_cache_free(m->d_xyz);
  dev_cache_free(m->d_cell_addr);
  dev_cache_free(m->d_cell_count);
  delete m;
}

extern "C" pcgx_status pcgx_sac_plane_model_create(const pcgx_bucket_grid *g, const void *data, int64_t n, int32_t stride,
                                                   int32_t xyz_off, int32_t on_device, pcgx_sac_plane_model **out) {
  PCGX_API_LOCK();
  if (!out) return fail(PCGX_E_INVALID, "pcgx_sac_plane_model_create: out is NULL");
  *out = nullptr;
  if (!g || n < 0 || (n > 0 && !data)) return fail(PCGX_E_INVALID, "pcgx_sac_plane_model_create: bad argument");
  if (n > 0 && (stride < 12 || xyz_off < 0 || xyz_off + 12 > stride))
    return fail(PCGX_E_BAD_FIELD, "pcgx_sac_plane_model_create: stride %d / xyz offset %d do not hold an xyz triple", stride,
                xyz_off);
  if (n > 0x7fffffffll) return fail(PCGX_E_TOO_LARGE, "pcgx_sac_plane_model_create: more than 2^31-1 points");
  PCGX_TRY(ensure_init());
  pcgx_sac_plane_model *m = new pcgx_sac_plane_model();
  m->n = n;
  m->gp = g->gp;
  m->resolution = g->resolution;
  for (int k = 0; k < 3; k++) {  // vg.MinMax() (voxelgrid.go:25-31), vgSize = vgMax - vgMin
    m->vg_min[k] = g->gp.origin[k];
    const float vmax = g->gp.origin[k] + (float)g->gp.size[k] * g->resolution;
    m->vg_size[k] = vmax - m->vg_min[k];
  }
  m->m = (int64_t)g->cell_addr.size();
  hipStream_t st = ctx().stream;
  Arena &ar = ctx().arena;
  auto body = [&]() -> pcgx_status {
    std::vector<uint32_t> counts((size_t)m->m);
    for (size_t c = 0; c < counts.size(); c++) counts[c] = g->cell_start[c + 1] - g->cell_start[c];
    PCGX_HIP_TRY(dev_cache_alloc((void **)&m->d_xyz, (size_t)n * sizeof(float4)));
    PCGX_HIP_TRY(dev_cache_alloc((void **)&m->d_cell_addr, (size_t)m->m * 4));
    PCGX_HIP_TRY(dev_cache_alloc((void **)&m->d_cell_count, (size_t)m->m * 4));
    PCGX_TRY(ar.begin(st));
    if (m->m > 0) {
      PCGX_HIP_TRY(hipMemcpyAsync(m->d_cell_addr, g->cell_addr.data(), (size_t)m->m * 4, hipMemcpyHostToDevice, st));
      PCGX_HIP_TRY(hipMemcpyAsync(m->d_cell_count, counts.data(), (size_t)m->m * 4, hipMemcpyHostToDevice, st));
    }
    if (n > 0) {
      const uint8_t *src = (const uint8_t *)data;
      if (!on_device) {
        uint8_t *d_raw = nullptr;
        PCGX_TRY(ar.alloc_n((size_t)n * stride, &d_raw));
        PCGX_HIP_TRY(hipMemcpyAsync(d_raw, data, (size_t)n * stride, hipMemcpyHostToDevice, st));
        src = d_raw;
      }
      hipLaunchKernelGGL(sac_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, n, stride, xyz_off,
                         m->d_xyz);
      PCGX_HIP_TRY(hipGetLastError());
    }
    // the caller's buffers (host or device) are free to change once this returns
    PCGX_HIP_TRY(hipStreamSynchronize(st));
    return PCGX_OK;
  };
  const pcgx_status rc = body();
  if (rc != PCGX_OK) {
    (void)hipStreamSynchronize(st);
    model_release(m);
    return rc;
  }
  *out = m;
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_sac_plane_model_free(pcgx_sac_plane_model *m) {
  PCGX_API_LOCK();
  model_release(m);  // (every call that used the model waited for its work before it returned)
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_sac_plane_compute(pcgx_sac_plane_model *m, const int64_t *ids, int64_t n, int32_t *found,
                                              int64_t *best, int64_t *best_score, pcgx_sac_plane *best_coeff,
                                              int32_t *ok, pcgx_sac_plane *coeff, int64_t *score) {
  PCGX_API_LOCK();
  if (!m || !found || !best || !best_score || !best_coeff || n < 0 || (n > 0 && !ids))
    return fail(PCGX_E_INVALID, "pcgx_sac_plane_compute: bad argument");
  if (n > 0x7fffffffll) return fail(PCGX_E_TOO_LARGE, "pcgx_sac_plane_compute: more than 2^31-1 hypotheses");
  for (int64_t i = 0; i < 3 * n; i++)
    if (ids[i] < 0 || ids[i] >= m->n)
      return fail(PCGX_E_OUT_OF_RANGE, "pcgx_sac_plane_compute: id %lld (sample %lld) outside [0, %lld) (the reference panics)",
                  (long long)ids[i], (long long)i, (long long)m->n);
  if (n == 0) {  // sac.go:53-55
    *found = 0;
    *best = -1;
    *best_score = 0;
    return PCGX_OK;
  }
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ar = ctx().arena;
  PCGX_TRY(ar.begin(st));
  const bool lds_bits = m->m <= kLdsBitmapCells;
  const int64_t slot_words = lds_bits ? 0 : (m->m + 31) / 32;
  int64_t groups = std::min<int64_t>(n, (int64_t)ctx().num_cu * (lds_bits ? 1 : 2));
  if (!lds_bits) groups = std::max<int64_t>(1, std::min<int64_t>(groups, ((int64_t)1 << 28) / slot_words));  // <= 1 GiB of bits
  uint32_t *d_ids = nullptr, *d_ext = nullptr, *d_slots = nullptr;
  int32_t *d_ok = nullptr;
  pcgx_sac_plane *d_coeff = nullptr;
  int64_t *d_score = nullptr;
  uint64_t *d_words = nullptr;  // {best, counter | too_large << 32}
  PCGX_TRY(ar.alloc_n((size_t)(3 * n), &d_ids));
  PCGX_TRY(ar.alloc_n((size_t)(2 * n), &d_ext));
  PCGX_TRY(ar.alloc_n((size_t)n, &d_ok));
  PCGX_TRY(ar.alloc_n((size_t)n, &d_coeff));
  PCGX_TRY(ar.alloc_n((size_t)n, &d_score));
  PCGX_TRY(ar.alloc_n(2, &d_words));
  if (!lds_bits) PCGX_TRY(ar.alloc_n((size_t)(groups * slot_words), &d_slots));
  std::vector<uint32_t> h_ids((size_t)(3 * n));
  for (int64_t i = 0; i < 3 * n; i++) h_ids[(size_t)i] = (uint32_t)ids[i];
  PCGX_HIP_TRY(hipMemcpyAsync(d_ids, h_ids.data(), (size_t)(3 * n) * 4, hipMemcpyHostToDevice, st));
  PCGX_HIP_TRY(hipMemsetAsync(d_words, 0, 16, st));
  if (!lds_bits) PCGX_HIP_TRY(hipMemsetAsync(d_slots, 0, (size_t)(groups * slot_words) * 4, st));
  uint32_t *counter = (uint32_t *)(d_words + 1), *too_large = counter + 1;
  SacFitArgs fa;
  fa.xyz = m->d_xyz;
  fa.ids = d_ids;
  fa.n = n;
  for (int k = 0; k < 3; k++) {
    fa.vg_min[k] = m->vg_min[k];
    fa.vg_size[k] = m->vg_size[k];
  }
  fa.resolution = m->resolution;
  fa.ok = d_ok;
  fa.coeff = d_coeff;
  fa.ext = d_ext;
  fa.score = d_score;
  fa.too_large = too_large;
  hipLaunchKernelGGL(sac_fit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, fa);
  SacEvalArgs ea;
  ea.gp = m->gp;
  ea.cell_addr = m->d_cell_addr;
  ea.cell_count = m->d_cell_count;
  ea.m = m->m;
  ea.ok = d_ok;
  ea.coeff = d_coeff;
  ea.ext = d_ext;
  ea.n = n;
  ea.counter = counter;
  ea.slots = d_slots;
  ea.slot_words = slot_words;
  ea.score = d_score;
  ea.best = (unsigned long long *)d_words;
  if (lds_bits)
    hipLaunchKernelGGL(sac_evaluate_kernel<true>, dim3((unsigned)groups), dim3(kSacEvalBlock), 0, st, ea);
  else
    hipLaunchKernelGGL(sac_evaluate_kernel<false>, dim3((unsigned)groups), dim3(kSacEvalBlock), 0, st, ea);
  PCGX_HIP_TRY(hipGetLastError());
  uint64_t words[2];
  PCGX_HIP_TRY(hipMemcpyAsync(words, d_words, 16, hipMemcpyDeviceToHost, st));
  PCGX_HIP_TRY(hipStreamSynchronize(st));
  if ((uint32_t)(words[1] >> 32))
    return fail(PCGX_E_TOO_LARGE, "pcgx_sac_plane_compute: a hypothesis' lattice has more than %d values along an axis",
                kSacSeqCap);
  pcgx_sac_plane bc;
  const int64_t bi = words[0] ? (int64_t)(0xffffffffu - (uint32_t)words[0]) : -1;
  if (bi >= 0) PCGX_HIP_TRY(hipMemcpyAsync(&bc, d_coeff + bi, sizeof(bc), hipMemcpyDeviceToHost, st));
  if (ok) PCGX_HIP_TRY(hipMemcpyAsync(ok, d_ok, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (coeff) PCGX_HIP_TRY(hipMemcpyAsync(coeff, d_coeff, (size_t)n * sizeof(pcgx_sac_plane), hipMemcpyDeviceToHost, st));
  if (score) PCGX_HIP_TRY(hipMemcpyAsync(score, d_score, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  PCGX_HIP_TRY(hipStreamSynchronize(st));
  *found = bi >= 0 ? 1 : 0;
  *best = bi;
  *best_score = bi >= 0 ? (int64_t)(words[0] >> 32) : 0;
  if (bi >= 0) *best_coeff = bc;
  return PCGX_OK;
}

extern "C" pcgx_status pcgx_sac_plane_inliers(pcgx_sac_plane_model *m, const pcgx_sac_plane *c, float d, int64_t *out,
                                              int64_t cap, int64_t *count) {
  PCGX_API_LOCK();
  if (!m || !c || !count || cap < 0 || (cap > 0 && !out)) return fail(PCGX_E_INVALID, "pcgx_sac_plane_inliers: bad argument");
  *count = 0;
  if (m->n == 0) return PCGX_OK;
  PCGX_TRY(ensure_init());
  hipStream_t st = ctx().stream;
  Arena &ar = ctx().arena;
  PCGX_TRY(ar.begin(st));
  const int ntiles = (int)((m->n + kRunTile - 1) / kRunTile);
  uint32_t *tile_count = nullptr, *d_total = nullptr;
  int64_t *d_out = nullptr;
  PCGX_TRY(ar.alloc_n((size_t)ntiles, &tile_count));
  PCGX_TRY(ar.alloc_n(1, &d_total));
  PCGX_TRY(ar.alloc_n((size_t)m->n, &d_out));
  SacInlierArgs A;
  A.xyz = m->d_xyz;
  A.n = m->n;
  for (int k = 0; k < 3; k++) {
    A.vg_min[k] = m->vg_min[k];
    A.norm[k] = c->norm[k];
  }
  A.dp = c->d;
  A.d = d;
  hipLaunchKernelGGL(sac_inliers_count_kernel, dim3(ntiles), dim3(256), 0, st, A, tile_count);
  hipLaunchKernelGGL(sac_inliers_scan_kernel, dim3(1), dim3(1024), 0, st, tile_count, ntiles, d_total);
  hipLaunchKernelGGL(sac_inliers_write_kernel, dim3(ntiles), dim3(256), 0, st, A, (const uint32_t *)tile_count, d_out);
  PCGX_HIP_TRY(hipGetLastError());
  uint32_t total = 0;
  PCGX_HIP_TRY(hipMemcpyAsync(&total, d_total, 4, hipMemcpyDeviceToHost, st));
  PCGX_HIP_TRY(hipStreamSynchronize(st));
  const int64_t k = std::min<int64_t>(total, cap);
  if (k > 0) {
    PCGX_HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    PCGX_HIP_TRY(hipStreamSynchronize(st));
  }
  *count = total;
  return PCGX_OK;
}

// IsIn(p, d) (surface.go:237-240), on the host
extern "C" pcgx_status pcgx_sac_plane_is_in(const pcgx_sac_plane_model *m, const pcgx_sac_plane *c, const float p[3], float d,
                                            int32_t *in) {
  PCGX_API_LOCK();
  if (!m || !c || !p || !in) return fail(PCGX_E_INVALID, "pcgx_sac_plane_is_in: NULL argument");
  const float q0 = p[0] - m->vg_min[0], q1 = p[1] - m->vg_min[1], q2 = p[2] - m->vg_min[2];
  const float dd = (c->norm[0] * q0 + c->norm[1] * q1 + c->norm[2] * q2) - c->d;
  *in = (-d < dd && dd < d) ? 1 : 0;
  return PCGX_OK;
}
