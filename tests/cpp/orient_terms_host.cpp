// csrc/orient_terms.h on the host (tests/test_orient_terms_host.py): the expressions the kernels compile, as a program
// of its own, built with -fsanitize=address,undefined.  It reads a table of edges from stdin,
//   first line: k            k edges
//   k lines:    i j a0 a1 a2 b0 b1 b2     the ids and the two normals, each component as 8 hex digits of its float32
// and prints per edge: c(i, j) and c(j, i) as 16 hex digits each, s, the weight key, the pair word seen from i and seen
// from j (hex); then k lines of k digits: before(e, f); then the node word checks, the anchor keys of a few heights, and
// the result of hooking and jumping random forests in random orders.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "orient_terms.h"

using namespace pcgx;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

static void shuffle(std::vector<uint32_t> &v) {
  for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[rnd() % (uint32_t)i]);
}

// A forest of n nodes grown in batches as the kernels grow it: on flat words, a batch of hooks (each root at most once,
// towards whatever the other end's word names, no cycle), then jump steps in a random node order until every word names
// a root.  The parity of every node relative to its root must be the XOR of the signs along the tree path: checked
// against signs propagated over the edge list.  Returns the number of nodes that disagree.
static int forest_trial(const uint32_t n, const int batches) {
  std::vector<uint32_t> word(n), ref_root(n), ref_par(n, 0u);
  for (uint32_t i = 0; i < n; i++) {
    word[i] = orient_node(i, 0u);
    ref_root[i] = i;
  }
  std::vector<uint32_t> order(n);
  for (uint32_t i = 0; i < n; i++) order[i] = i;
  for (int b = 0; b < batches; b++) {
    // every root draws an edge (a under it, b anywhere); it hooks if that makes no cycle among this batch's hooks
    std::vector<uint32_t> members(n);
    for (uint32_t i = 0; i < n; i++) members[i] = i;
    shuffle(members);
    std::vector<uint32_t> batch_root = ref_root;  // union-find over this batch, by reference roots
    auto find = [&](uint32_t x) {
      while (batch_root[x] != x) x = batch_root[x] = batch_root[batch_root[x]];
      return x;
    };
    std::vector<uint8_t> hooked(n, 0);
    for (uint32_t t = 0; t < n; t++) {
      const uint32_t a = members[t], bnode = rnd() % n, s = rnd() & 1u;
      const uint32_t A = orient_parent(word[a]);
      if (hooked[A] || orient_parent(word[A]) != A) continue;  // (a's word is flat: A was a root when the batch began)
      if (find(A) == find(ref_root[bnode])) continue;
      const uint32_t wa = a == A ? orient_node(A, 0u) : word[a], wb = word[bnode];  // (wb may be a word hooked a moment ago)
      batch_root[find(A)] = find(ref_root[bnode]);
      hooked[A] = 1;
      word[A] = orient_hook_word(orient_parent(wb), orient_parity(wa), s, orient_parity(wb));
      // the reference: everything under A changes side by par(a) ^ s ^ par_ref(b) and joins b's component
      const uint32_t shift = ref_par[a] ^ s ^ ref_par[bnode], to = ref_root[bnode];
      for (uint32_t i = 0; i < n; i++)
        if (ref_root[i] == A) {
          ref_par[i] ^= shift;
          ref_root[i] = to;
        }
    }
    // the reference's roots are arbitrary names; rename every component to the root the words will reach
    for (;;) {
      bool moved = false;
      shuffle(order);
      for (uint32_t k = 0; k < n; k++) {
        const uint32_t i = order[k], w = word[i], p = orient_parent(w);
        if (p == i) continue;
        const uint32_t wp = word[p];
        if (orient_parent(wp) == p) continue;
        word[i] = orient_jump(w, wp);
        moved = true;
      }
      if (!moved) break;
    }
    // ref_par is relative to the reference's root name `to`, the words' to the real root: both differ by a constant
    // per component, the parity of `to` under the real root
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t real = orient_parent(word[i]);
      if (ref_root[i] != real) {
        const uint32_t old = ref_root[i], shift = ref_par[real];
        for (uint32_t j = 0; j < n; j++)
          if (ref_root[j] == old) {
            ref_root[j] = real;
            ref_par[j] ^= shift;
          }
      }
    }
  }
  int bad = 0;
  for (uint32_t i = 0; i < n; i++)
    if (orient_parent(word[i]) != ref_root[i] || orient_parity(word[i]) != ref_par[i]) bad++;
  return bad;
}

int main() {
  long long k = 0;
  if (scanf("%lld", &k) != 1 || k < 0) return 2;
  std::vector<OrientEdge> edges((size_t)k);
  for (long long r = 0; r < k; r++) {
    uint32_t i = 0, j = 0, bits[6];
    if (scanf("%" SCNu32 " %" SCNu32, &i, &j) != 2) return 2;
    float v[6];
    for (int c = 0; c < 6; c++) {
      if (scanf("%" SCNx32, &bits[c]) != 1) return 2;
      memcpy(&v[c], &bits[c], 4);
    }
    const double c0 = orient_c(v[0], v[1], v[2], v[3], v[4], v[5]), c1 = orient_c(v[3], v[4], v[5], v[0], v[1], v[2]);
    uint64_t b0, b1;
    memcpy(&b0, &c0, 8);
    memcpy(&b1, &c1, 8);
    edges[(size_t)r] = OrientEdge{orient_weight_key(c0), orient_pair(i, j)};
    printf("%016" PRIx64 " %016" PRIx64 " %u %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", b0, b1, orient_s(c0),
           orient_weight_key(c0), orient_pair(i, j), orient_pair(j, i));
  }
  for (long long r = 0; r < k; r++) {
    for (long long q = 0; q < k; q++) putchar(orient_before(edges[(size_t)r], edges[(size_t)q]) ? '1' : '0');
    putchar('\n');
  }
  const OrientEdge none{0ull, kOrientNoPair};
  printf("none %d %d %d\n", k > 0 && orient_before(edges[0], none) ? 1 : 0, k > 0 && orient_before(none, edges[0]) ? 1 : 0,
         orient_before(none, none) ? 1 : 0);
  // node words and pair words at the largest id
  const uint32_t top = kOrientMaxId;
  int words_ok = 1;
  for (uint32_t par = 0; par < 2; par++) {
    const uint32_t w = orient_node(top, par);
    words_ok &= orient_parent(w) == top && orient_parity(w) == par;
    words_ok &= orient_jump(orient_node(5u, par), orient_node(top, 1u)) == orient_node(top, par ^ 1u);
    words_ok &= orient_hook_word(top, par, 1u, 1u) == orient_node(top, par);
  }
  const uint64_t pw = orient_pair(top, top - 1u);
  words_ok &= orient_pair_lo(pw) == top - 1u && orient_pair_hi(pw) == top && orient_pair_mine(pw) == top &&
              orient_pair_other(pw) == top - 1u && orient_same_edge(pw, orient_pair(top - 1u, top)) && pw != kOrientNoPair;
  printf("words %u %d\n", top, words_ok);
  const float hs[] = {-__builtin_inff(), -1.0f, -0.0f, 0.0f, 1e-45f, 1.0f, __builtin_inff()};
  for (float h : hs) printf("anchor %016" PRIx64 " %u\n", orient_anchor_key(h, 7u), orient_anchor_id(orient_anchor_key(h, 7u)));
  printf("flip %08x %08x %08x\n", orient_flip_bits(0x3f800000u, 1u), orient_flip_bits(0x7fc00001u, 1u),
         orient_flip_bits(0x80000000u, 0u));
  printf("votes %d %d %d %u %u\n", orient_vote(0, 0, 1, 0u, 0, 0, 0, 0, 0, 5), orient_vote(0, 0, 1, 1u, 0, 0, 0, 0, 0, 5),
         orient_vote(1, 0, 0, 0u, 0, 0, 0, 0, 0, 5), orient_vote_sigma(orient_vote_word(-1) * 3 + orient_vote_word(1) * 2),
         orient_vote_sigma(orient_vote_word(-1) * 2 + orient_vote_word(1) * 2));
  printf("rounds %d %d %d %d %d\n", orient_full_rounds(1), orient_full_rounds(2), orient_full_rounds(3),
         orient_full_rounds(4096), orient_full_rounds(4097));
  int bad = 0;
  for (int trial = 0; trial < 6; trial++) bad += forest_trial(1000u, 1 + trial);
  printf("forests %d\n", bad);
  return 0;
}
