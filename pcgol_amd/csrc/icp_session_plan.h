// What an ICP session is and what it holds, decided in one place: plan_session() maps the facts of a session at its
// creation (SessionFacts) to its kind, the sums it forms, whether it is a one-launch session and the size of every buffer
// it allocates (SessionPlan).  Plain C++ on host values: no HIP, no session or tree type, no environment -- icp.hip
// gathers the facts, reads the environment and the knob, asks small_fit_eligible / small_fit_wants_order / icp_grid, and
// builds what the plan says (session_create); tests/test_icp_session_plan.py compiles this header with g++ and compares
// the plan over the whole input space.  OwnedBlocks, below, is how a session frees what it was given.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pcgx {

// workgroup sizes the sizes below depend on: icp_grid_kernel (with sums) and icp_gicp_sums_kernel
constexpr int kIcpGridBlock = 256;
constexpr int kGicpBlock = 256;

struct SessionFacts {
  bool normals = false;           // base normals were given: a point-to-plane session
  bool covariances = false;       // base covariances were given: a GICP session
  int32_t sums_mode = 0;          // PCGX_SUMS_*: 0 the reference's sums, 1 float64, 2 the reference's sums by one wave
  int32_t strict_override = -1;   // PCGX_ICP_STRICT: -1 not set, else 1 / 2 by its first character, anything else 0
  int64_t nt = 0;                 // targets
  int64_t n_base = 1;             // the base's points, deleted ones included: normals and covariances go by original id
  bool patched = false;           // the base has deletions: the reference's patched explicit tree is walked
  bool has_nan = false;           // the base has NaN points
  bool small_on = true;           // PCGX_ICP_SMALL
  bool small_eligible = false;    // small_fit_eligible's answer
  bool small_wants_order = false; // small_fit_wants_order's answer
  int32_t grid = 1;               // icp_grid's answer: the launch grid of the walk
  int32_t num_cu = 1;             // compute units of the device
  bool caller_sums = false;       // the caller supplied d_sums
  size_t state_bytes = 0;         // sizeof(IcpState)
};

enum SessionBuffer : int32_t {  // (the order they are allocated in)
  kBufXyz, kBufState, kBufPartials, kBufPosOf, kBufMatch, kBufMatchCert, kBufFirstLeaf, kBufWalkList, kBufWalkCount,
  kBufSums, kBufMatchId, kBufNormals, kBufBaseCov, kBufTargetCov, kBufDropped, kBufValid, kBufSmallPerm,
  kSessionBuffers
};

struct SessionPlan {
  bool gicp = false;
  bool plane = false;            // point-to-plane or GICP: 30 sums, the Gauss-Newton update
  int32_t strict = 0;            // the reference's sequential float32 sums: 1 = strict.hip, 2 = the one-wave chain
  bool strict_explicit = false;  // ... asked for by name
  bool small = false;            // both clouds small: a step, or a whole Fit, is one launch (icp_small.hip)
  int32_t gicp_grid = 1;         // workgroups of icp_gicp_sums_kernel = its rows of d_partials
  int32_t n_sums = 10;
  // the general path's start values are written at creation (reset_state, general_prepare); a small session leaves them
  // to its first step outside the one launch, and small_fit_prepare writes its own
  bool start_values = true;
  int64_t nt_pad = 0;            // small: nt rounded up to whole waves (else set by the first strict 2 step)
  bool small_buffers = false;    // d_terms and d_small_sync exist (small_fit_terms_bytes, small_fit_sync_bytes)
  size_t bytes[kSessionBuffers] = {};  // per SessionBuffer; 0: not allocated
};

inline SessionPlan plan_session(const SessionFacts &f) {
  SessionPlan p;
  p.gicp = f.covariances;
  p.plane = f.normals || p.gicp;
  // the reference's own sums unless the caller asks otherwise (include/pcgx.h, PCGX_SUMS_*); the point-to-plane and GICP
  // extensions have no reference sums to reproduce
  p.strict = p.plane ? 0 : (f.sums_mode == 0 ? 1 : (f.sums_mode == 1 ? 0 : 2));
  p.strict_explicit = p.strict == 2;
  if (f.strict_override >= 0) {  // experiments: overrides sums_mode
    p.strict = p.plane ? 0 : f.strict_override;
    p.strict_explicit = p.strict != 0;
  }
  p.n_sums = p.plane ? 30 : 10;
  if (p.gicp) {
    const int64_t g = (f.nt + kGicpBlock - 1) / kGicpBlock, cap = (int64_t)f.num_cu * 8;
    p.gicp_grid = (int32_t)(g < 1 ? 1 : (g > cap ? cap : g));
  }
  // Small clouds (the reference's own benchmark shapes, icp_test.go:100-142): the whole Fit in one launch
  // (icp_small.hip), the target in the caller's order -- the sums run in that order.
  p.small = f.small_on && f.nt > 0 && !p.plane && !f.patched && p.strict == 1 && !f.has_nan && f.small_eligible;
  p.start_values = !p.small;
  const size_t n1 = (size_t)(f.nt ? f.nt : 1), nb = (size_t)f.n_base;
  p.bytes[kBufXyz] = n1 * 12;  // SoA x | y | z
  p.bytes[kBufState] = f.state_bytes;
  // a row per workgroup of the walk, of the grid pass and (GICP) of the sums kernel
  p.bytes[kBufPartials] = ((size_t)f.grid + (size_t)(f.nt / kIcpGridBlock) + 1 + (size_t)(p.gicp ? p.gicp_grid : 0)) *
                          p.n_sums * sizeof(double);
  p.bytes[kBufPosOf] = n1 * sizeof(uint32_t);
  p.bytes[kBufMatch] = n1 * 16;  // float4
  p.bytes[kBufMatchCert] = n1 * sizeof(float);
  p.bytes[kBufFirstLeaf] = n1 * sizeof(uint32_t);
  p.bytes[kBufWalkList] = n1 * sizeof(uint32_t);
  p.bytes[kBufWalkCount] = (size_t)f.grid * sizeof(uint32_t);
  p.bytes[kBufSums] = f.caller_sums ? 0 : (size_t)p.n_sums * sizeof(double);
  p.bytes[kBufMatchId] = p.plane ? n1 * sizeof(uint32_t) : 0;
  p.bytes[kBufNormals] = p.plane && !p.gicp ? nb * 16 : 0;  // float4 per base id
  if (p.gicp) {
    p.bytes[kBufBaseCov] = nb * 2 * 16;   // two float4 per base id
    p.bytes[kBufTargetCov] = n1 * 3 * 8;  // three float2 per target
    p.bytes[kBufDropped] = (size_t)p.gicp_grid * sizeof(uint32_t);
  }
  if (p.small) {
    p.small_buffers = true;
    p.nt_pad = (f.nt + 63) & ~(int64_t)63;
    p.bytes[kBufValid] = (size_t)(p.nt_pad / 64) * sizeof(unsigned long long);
    p.bytes[kBufSmallPerm] = f.small_wants_order ? (size_t)f.nt * sizeof(int32_t) : 0;
  }
  return p;
}

// The blocks an object owns, each with the function that gives it back: what was adopted is released exactly once, by
// release_all() (the object's end, or a creation that failed half way) or earlier by give_up().
class OwnedBlocks {
 public:
  using Release = void (*)(void *);
  void adopt(void *p, Release release) {
    if (p) blocks_.push_back({p, release});
  }
  // released now and forgotten (one of a pair of buffers, the other could not be had); a block not owned is left alone
  void give_up(void *p) {
    for (auto it = blocks_.begin(); it != blocks_.end(); ++it)
      if (it->p == p) {
        it->release(p);
        blocks_.erase(it);
        return;
      }
  }
  void release_all() {
    for (const Block &b : blocks_) b.release(b.p);
    blocks_.clear();
  }

 private:
  struct Block {
    void *p;
    Release release;
  };
  std::vector<Block> blocks_;
};

}  // namespace pcgx
