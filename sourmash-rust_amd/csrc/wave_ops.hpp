// wave_ops.hpp -- reductions over the 64 lanes of a wave, the result in every lane's return value.  Shared by the kernels
// that end a per-lane count with one (angular, compare, gather, gather_many, match, sbt, sigtext).  No state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smh {

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  for (int off = 32; off; off >>= 1) { const uint64_t o = __shfl_xor(v, off); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
  for (uint32_t d = 32; d; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d, 64);
  return x;
}

}  // namespace smh
