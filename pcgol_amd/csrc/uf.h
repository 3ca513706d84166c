// uf.h -- the lock-free union-find of the component kernels (segment.hip: flood fill; radius_graph.h: the radius graph's
// components for region growing, clusters and DBSCAN), one statement of it for all.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pcgx {

// ------------------------------------------------------------------ union-find
// parent[x] <= x always: roots are hooked under smaller roots only and paths are compressed
// towards ancestors, so the root of a finished component is its smallest member.
__device__ __forceinline__ uint32_t uf_load(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__device__ __forceinline__ uint32_t uf_find(uint32_t *__restrict__ parent, uint32_t x) {
  for (;;) {
    const uint32_t p = uf_load(parent + x);
    if (p == x) return x;
    const uint32_t gp = uf_load(parent + p);
    // path halving with a plain store: whatever another thread writes here at the same time is an ancestor of x
    // too (parents only ever move towards the root), so either value keeps the structure -- and an atomic per hop
    // is what the finds used to cost
    if (gp != p) __atomic_store_n(parent + x, gp, __ATOMIC_RELAXED);
    x = p;
  }
}

__device__ __forceinline__ void uf_union(uint32_t *__restrict__ parent, uint32_t a, uint32_t b) {
  a = uf_find(parent, a);
  b = uf_find(parent, b);
  while (a != b) {
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicCAS(parent + a, a, b);  // hook the larger root under the smaller
    if (old == a) return;
    a = uf_find(parent, old);
    b = uf_find(parent, b);
  }
}

// An edge from a point last seen under my_root to j: union if j's root differs; returns a root the point is under now.
__device__ __forceinline__ uint32_t uf_link(uint32_t *__restrict__ parent, uint32_t my_root, const uint32_t j) {
  const uint32_t rj = uf_find(parent, j);
  if (rj != my_root) {
    uf_union(parent, my_root, rj);
    my_root = uf_find(parent, my_root);
  }
  return my_root;
}

// parent[i] := root of i (every chain descends: roots are their components' smallest members so far)
// (static: each source file that includes this launches its own copy)
static __global__ __launch_bounds__(256) void uf_jump_kernel(uint32_t *__restrict__ parent, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t r = uf_load(parent + i);
  for (;;) {
    const uint32_t p = uf_load(parent + r);
    if (p == r) break;
    r = p;
  }
  __atomic_store_n(parent + i, r, __ATOMIC_RELAXED);
}

}  // namespace pcgx
