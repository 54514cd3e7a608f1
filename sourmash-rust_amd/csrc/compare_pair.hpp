// compare_pair.hpp -- the per-pair union walk of the compare kernels (reference src/lib.rs:428-436, 470-508), shared by
// compare_kernels.hip (k_compare_wave and the kernels built on `walk`) and sbt_kernels.hip (the SBT's leaf pairs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_ops.hpp"

namespace smh {
namespace {

struct PairCounts {
  uint32_t uni;  // new union elements in my diagonal
  uint32_t com;  // elements of B that duplicate an element of A in my diagonal
};

// A and B may live in LDS or global memory; the walk is identical.
template <bool Count>
__device__ __forceinline__ PairCounts walk(const uint64_t* A, uint32_t la, const uint64_t* B,
                                           uint32_t lb, uint32_t pa, uint32_t pb, uint32_t steps,
                                           uint64_t u0, uint64_t n) {
  // Count == false: plain census.  Count == true: `com` only counts duplicates whose union rank
  // (running union count, the duplicate itself adds none) is <= n.
  uint32_t uni = 0, com = 0;
  for (uint32_t t = 0; t < steps; t++) {
    bool takeA = (pb >= lb) || (pa < la && A[pa] <= B[pb]);
    if (takeA) { pa++; uni++; }
    else {
      bool dup = pa > 0 && A[pa - 1] == B[pb];
      if (dup) { if (!Count || u0 + uni <= n) com++; }
      else uni++;
      pb++;
    }
  }
  return {uni, com};
}

__device__ __forceinline__ uint64_t wave_excl_scan64(uint64_t v, int lane) {
  uint64_t incl = v;
  for (int off = 1; off < 64; off <<= 1) {
    uint64_t o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  return incl - v;
}

struct PairResult64 {
  uint64_t common;  // elements of both within the first n of the union (n == 0: unbounded)
  uint64_t size;    // union elements walked: min(|A u B|, n)
  uint64_t tot_c;   // |A ^ B| untruncated
};

// One ordered pair (A = self, whose num truncates) walked by one whole wavefront; every lane gets the result.  The merged
// sequence (ties: A first) is cut into 64 equal diagonals by a merge-path binary search, every lane walks its diagonal,
// and a wave prefix sum over the per-lane union counts places the truncation point.
__device__ __forceinline__ PairResult64 wave_compare_pair(const uint64_t* A, uint32_t la, const uint64_t* B, uint32_t lb,
                                                          uint64_t n, int lane) {
  const uint32_t total = la + lb;
  const uint32_t D = (total + 63) / 64;
  const uint32_t t0 = min((uint32_t)lane * D, total), t1 = min(t0 + D, total);
  // merge path: pa = how many of the first t0 merged elements come from A (ties: A first)
  uint32_t lo = t0 > lb ? t0 - lb : 0, hi = min(t0, la);
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (A[mid] <= B[t0 - 1 - mid]) lo = mid + 1; else hi = mid;
  }
  const uint32_t pa = lo, pb = t0 - lo;
  PairCounts c = walk<false>(A, la, B, lb, pa, pb, t1 - t0, 0, 0);
  const uint64_t u0 = wave_excl_scan64(c.uni, lane);
  const uint64_t tot_u = wave_sum_u64(c.uni);
  const uint64_t tot_c = wave_sum_u64(c.com);
  uint64_t mine = c.com;
  if (n != 0 && tot_u > n) {
    if (u0 + c.uni <= n) mine = c.com;
    else if (u0 <= n) mine = walk<true>(A, la, B, lb, pa, pb, t1 - t0, u0, n).com;
    else mine = 0;
  }
  PairResult64 r;
  r.common = wave_sum_u64(mine);
  r.size = (n != 0 && tot_u > n) ? n : tot_u;
  r.tot_c = tot_c;
  return r;
}

}  // namespace
}  // namespace smh
