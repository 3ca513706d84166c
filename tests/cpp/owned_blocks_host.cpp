// OwnedBlocks (csrc/icp_session_plan.h) over a stub allocator, as a program of its own (tests/test_icp_session_plan.py
// builds and runs it; it is small enough to run under the host sanitizers too): what a session adopts is released once.
#include <cstdio>
#include <cstdlib>
#include <map>

#include "icp_session_plan.h"

using namespace pcgx;

static std::map<void *, int> g_freed;  // block -> times released
static int g_live = 0, g_other = 0, g_fail_at = -1, g_allocs = 0;

static int stub_alloc(void **p, size_t bytes) {  // (dev_cache_alloc's shape: 0 is success)
  *p = nullptr;
  if (g_allocs++ == g_fail_at) return 2;
  *p = malloc(bytes);
  g_freed[*p] = 0;
  g_live++;
  return 0;
}
static void stub_free(void *p) {
  if (!p) return;  // (dev_cache_free(nullptr) is allowed)
  if (++g_freed[p] == 1) g_live--;  // (the memory is kept until reset(): no address comes twice in one scenario)
}
static void other_free(void *p) {  // a block with a release function of its own (the strict sums' buffers)
  g_other++;
  stub_free(p);
}

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #c);  \
      return 1;                                                     \
    }                                                               \
  } while (0)

static bool all_freed_once() {
  for (const auto &kv : g_freed)
    if (kv.second != 1) return false;
  return g_live == 0;
}
static void reset(int fail_at) {
  for (const auto &kv : g_freed) free(kv.first);
  g_freed.clear();
  g_live = g_other = g_allocs = 0;
  g_fail_at = fail_at;
}
static int take(OwnedBlocks &o, void **p, size_t bytes, OwnedBlocks::Release r = stub_free) {
  const int e = stub_alloc(p, bytes);
  if (e == 0) o.adopt(*p, r);
  return e;
}

int main() {
  {  // every owned block is freed once, each by its own function; a second release_all frees nothing again
    reset(-1);
    OwnedBlocks o;
    void *p[20];
    for (int k = 0; k < 20; k++) CHECK(take(o, &p[k], 16 + k, k == 7 ? other_free : stub_free) == 0);
    o.adopt(nullptr, stub_free);  // (a buffer the plan gave no size: nothing to own)
    CHECK(g_live == 20);
    o.release_all();
    CHECK(all_freed_once() && g_freed.size() == 20 && g_other == 1);
    o.release_all();
    CHECK(all_freed_once() && g_other == 1);
  }
  {  // decide_step's "could not get both, go on without": the first of a pair came, the second did not
    reset(3);
    OwnedBlocks o;
    void *a = nullptr, *b = nullptr, *c = nullptr, *orig_of = nullptr, *match_caller = nullptr, *later = nullptr;
    CHECK(take(o, &a, 64) == 0 && take(o, &b, 64) == 0 && take(o, &orig_of, 64) == 0);
    CHECK(take(o, &match_caller, 64) != 0 && match_caller == nullptr);
    o.give_up(orig_of);
    o.give_up(match_caller);  // (never owned: left alone)
    CHECK(g_freed[orig_of] == 1 && g_live == 2);
    o.give_up(orig_of);  // (no longer owned: not freed twice)
    CHECK(g_freed[orig_of] == 1);
    CHECK(take(o, &later, 64) == 0);  // the session goes on: blocks made after that are owned like the others
    int local = 0;
    c = &local;
    o.give_up(c);  // a pointer that was never adopted is not released
    CHECK(g_live == 3);
    o.release_all();
    CHECK(all_freed_once() && g_freed.size() == 4);
  }
  for (int fail_at = 0; fail_at < 6; fail_at++) {  // a creation that fails at its k-th buffer frees the k it got
    reset(fail_at);
    OwnedBlocks o;
    void *p[6] = {};
    int e = 0, got = 0;
    for (int k = 0; k < 6 && e == 0; k++)
      if ((e = take(o, &p[k], 128)) == 0) got++;
    CHECK(e != 0 && got == fail_at && g_live == got);
    o.release_all();
    CHECK(all_freed_once() && (int)g_freed.size() == got);
  }
  reset(-1);
  printf("ok\n");
  return 0;
}
