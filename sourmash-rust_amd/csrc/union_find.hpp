// union_find.hpp -- the lock-free union-find in device memory shared by compare_kernels.hip (the components of the "shares a
// hash" graph) and cluster_kernels.hip (single linkage).  parent[v] <= v always: the larger root goes under the smaller, so a
// root is its component's smallest node and the forest that any order of unions leaves has the same roots.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smh {
namespace {

__device__ __forceinline__ uint32_t uf_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // past the per-CU cache
}
__device__ __forceinline__ uint32_t uf_find(uint32_t* parent, uint32_t x) {
  uint32_t p = uf_load(parent + x);
  while (p != x) {
    const uint32_t gp = uf_load(parent + p);
    if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // halving: gp is an ancestor
    x = p; p = gp;
  }
  return x;
}
__device__ __forceinline__ void uf_union(uint32_t* parent, uint32_t x, uint32_t y) {
  while (true) {
    x = uf_find(parent, x); y = uf_find(parent, y);
    if (x == y) return;
    if (x > y) { const uint32_t t = x; x = y; y = t; }
    if (atomicCAS(parent + y, y, x) == y) return;   // the larger root goes under the smaller: parent[v] <= v always
  }
}

}  // namespace
}  // namespace smh
