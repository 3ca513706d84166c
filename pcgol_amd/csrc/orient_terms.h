// orient_terms.h -- the decisions of consistent normal orientation, shared by the device kernels (orient.hip) and the
// host test (tests/cpp/orient_terms_host.cpp): one expression, compiled by both.
// NOT in the reference: no parity, checked against the NumPy oracle's restatement (tests/orient_oracle.py).
//
// Contract (include/pcgx.h, "consistent normal orientation"): the flips are the sign parity along the minimum spanning
// forest of the radius graph on the usable points, its edges strictly ordered by (|c| descending, min id, max id), c
// cluster_terms.h's float64 dot product of the two normals.  The forest is grown in Boruvka rounds; what a round adds is
// a property of the point set, so nothing here depends on a schedule.
//
// The union-find that carries the parity.  A node word is {parent : 31, parity : 1}: parity is the XOR of the edge signs
// along the forest path from the node to `parent`.  INVARIANT: at every moment every word names the node itself or an
// ancestor of it in the union-find tree, together with the node's parity relative to THAT ancestor.  A hook writes a
// root's word once (orient_hook_word); a pointer jump replaces {p, s} by {p', s ^ s'} where {p', s'} is p's word
// (orient_jump).  If p's word is an ancestor-with-parity of p, the composition is one of the node, whichever of p's
// successive words the lane happened to read: a lane may read a word another lane has already flattened, or one a root
// wrote a moment ago, and the invariant still holds.  Words are 32 bits, loaded and stored whole.
#pragma once
#include "cluster_terms.h"

namespace pcgx {

// ids are below 2^31 - 1 (the node word keeps 31 bits of parent)
constexpr uint32_t kOrientMaxId = 0x7ffffffeu;

// The usable test: cluster_terms.h's rule with normals given and no curvature.
PCGX_HD bool orient_usable(const bool in_own_neighbourhood, const float nx, const float ny, const float nz) {
  return cluster_usable(in_own_neighbourhood, true, nx, ny, nz, false, 0.0f, 0.0f);
}

// The agreement of two normals: cluster_normals_agree's expression.  Symmetric in (i, j) bit for bit.
PCGX_HD double orient_c(const float nxi, const float nyi, const float nzi, const float nxj, const float nyj,
                        const float nzj) {
  return ((double)nxi * (double)nxj + (double)nyi * (double)nyj) + (double)nzi * (double)nzj;
}
// The sign of an edge: do the two normals point to opposite sides?  (-0: no)
PCGX_HD uint32_t orient_s(const double c) { return c < 0.0 ? 1u : 0u; }

// |c| as a word whose unsigned order is |c|'s (c is finite: the normals are), plus one: 0 is "no edge".
PCGX_HD uint64_t orient_weight_key(const double c) {
  const double a = fabs(c);
  uint64_t b;
  __builtin_memcpy(&b, &a, 8);
  return b + 1ull;
}

// An edge as a lane keeps it: the weight key and the pair word {lo : 31, hi : 32, mine_is_hi : 1}.  For the component
// that offers it the last bit is a function of the edge, so the order of pair words is the order of (lo, hi).
struct OrientEdge {
  uint64_t weight;  // 0: none
  uint64_t pair;
};
constexpr uint64_t kOrientNoPair = ~0ull;
PCGX_HD uint64_t orient_pair(const uint32_t mine, const uint32_t other) {
  const uint32_t lo = mine < other ? mine : other, hi = mine < other ? other : mine;
  return ((uint64_t)lo << 33) | ((uint64_t)hi << 1) | (uint64_t)(mine == hi ? 1u : 0u);
}
PCGX_HD uint32_t orient_pair_lo(const uint64_t pair) { return (uint32_t)(pair >> 33); }
PCGX_HD uint32_t orient_pair_hi(const uint64_t pair) { return (uint32_t)(pair >> 1) & 0x7fffffffu; }
PCGX_HD uint32_t orient_pair_mine(const uint64_t pair) { return (pair & 1ull) ? orient_pair_hi(pair) : orient_pair_lo(pair); }
PCGX_HD uint32_t orient_pair_other(const uint64_t pair) { return (pair & 1ull) ? orient_pair_lo(pair) : orient_pair_hi(pair); }
PCGX_HD bool orient_same_edge(const uint64_t p, const uint64_t q) { return (p >> 1) == (q >> 1); }

// The edge order: does e come before f?  The larger |c|, then the smaller min id, then the smaller max id.  Strict and
// total over distinct edges; an edge is not before itself; "no edge" comes after every edge.
PCGX_HD bool orient_before(const OrientEdge &e, const OrientEdge &f) {
  if (e.weight != f.weight) return e.weight > f.weight;
  return e.weight != 0ull && (e.pair >> 1) < (f.pair >> 1);
}

// The packed node word.
PCGX_HD uint32_t orient_node(const uint32_t parent, const uint32_t parity) { return (parent << 1) | (parity & 1u); }
PCGX_HD uint32_t orient_parent(const uint32_t word) { return word >> 1; }
PCGX_HD uint32_t orient_parity(const uint32_t word) { return word & 1u; }

// Root A hooks under `target`, an ancestor-or-self of b, through the edge (a, b) of sign s, a under A with parity
// par_a, b with parity par_b relative to target: A's parity relative to target.
PCGX_HD uint32_t orient_hook_word(const uint32_t target, const uint32_t par_a, const uint32_t s, const uint32_t par_b) {
  return orient_node(target, par_a ^ s ^ par_b);
}

// One pointer-jump step: the node's word and its parent's word -> the node's next word.
PCGX_HD uint32_t orient_jump(const uint32_t word, const uint32_t parent_word) {
  return orient_node(orient_parent(parent_word), orient_parity(word) ^ orient_parity(parent_word));
}

// A normal's component after a flip: the sign bit inverted, every other bit as given.
PCGX_HD uint32_t orient_flip_bits(const uint32_t bits, const uint32_t flip) { return bits ^ (flip << 31); }
PCGX_HD float orient_flipped(const float v, const uint32_t flip) {
  uint32_t b;
  __builtin_memcpy(&b, &v, 4);
  b = orient_flip_bits(b, flip);
  float r;
  __builtin_memcpy(&r, &b, 4);
  return r;
}

// Mode 1.  The height of a point along u, float32, never contracted; the anchor key: the height's order-preserving
// bits (h + 0 first, so that -0 ties with +0; a NaN from an overflow is ordered by its bits), then ~id: the largest key
// is the largest height, ties to the smallest id.
PCGX_HD float orient_height(const float px, const float py, const float pz, const float ux, const float uy, const float uz) {
  return (px * ux + py * uy) + pz * uz;
}
PCGX_HD uint64_t orient_anchor_key(const float h, const uint32_t id) {
  const float z = h + 0.0f;
  uint32_t b;
  __builtin_memcpy(&b, &z, 4);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((uint64_t)b << 32) | (uint64_t)(~id);
}
PCGX_HD uint32_t orient_anchor_id(const uint64_t key) { return ~(uint32_t)key; }
// Does the anchor's normal, after its parity, look against u?
PCGX_HD uint32_t orient_anchor_sigma(const float nx, const float ny, const float nz, const uint32_t parity, const float ux,
                                     const float uy, const float uz) {
  return orient_c(orient_flipped(nx, parity), orient_flipped(ny, parity), orient_flipped(nz, parity), ux, uy, uz) < 0.0
             ? 1u : 0u;
}

// Mode 2.  One member's vote on its normal after its parity: -1 "wrong" (looks away from the viewpoint), +1 "right",
// 0 abstains (t == 0, or a NaN from an overflow).
PCGX_HD int orient_vote(const float nx, const float ny, const float nz, const uint32_t parity, const float px, const float py,
                        const float pz, const float vx, const float vy, const float vz) {
  const double ex = (double)vx - (double)px, ey = (double)vy - (double)py, ez = (double)vz - (double)pz;
  const double t = ((double)orient_flipped(nx, parity) * ex + (double)orient_flipped(ny, parity) * ey) +
                   (double)orient_flipped(nz, parity) * ez;
  return t < 0.0 ? -1 : (t > 0.0 ? 1 : 0);
}
// votes packed {wrong : 32, right : 32}
PCGX_HD uint64_t orient_vote_word(const int vote) { return vote < 0 ? (1ull << 32) : (vote > 0 ? 1ull : 0ull); }
PCGX_HD uint32_t orient_vote_sigma(const uint64_t votes) { return (uint32_t)(votes >> 32) > (uint32_t)votes ? 1u : 0u; }

// Rounds that finish for certain: the components with a leaving edge at least halve each round.
PCGX_HD int32_t orient_full_rounds(const int64_t n) {
  int32_t r = 1;
  while (((int64_t)1 << r) < n) r++;
  return r;
}

}  // namespace pcgx
