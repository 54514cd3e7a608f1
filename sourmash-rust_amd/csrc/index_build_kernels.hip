// index_build_kernels.hip -- gfx950 kernels of building a resident index from records (include/sourmash_amd.h, "Building an
// index from records").  The hashing kernels and the two radix sorts leave the candidates of a fold ordered
// by (group, hash); what follows here turns them into the runs of a CSR with no host pass over runs or groups:
//
//   k_ib_heads    an element is a head when its group or its hash differs from its predecessor's (element 0 always is; the
//                 first element of a tile reads the last one of the tile in front of it).  One workgroup per tile of
//                 kBuildTile elements leaves the tile's number of heads; exclusive_scan_u32_dev turns them into where each
//                 tile's runs start.
//   k_ib_emit     the same pass again: a head's run number is its tile's start + the heads in front of it inside the tile
//                 (ballot / popcount inside a wave; the waves and steps of a workgroup in element order through 32 LDS
//                 words), so the runs come out in order with no cursor.  It writes the run's hash and where it starts.
//   k_ib_counts   one lane per run: its group, and its length -- or, when the elements are the runs of several folds, the
//                 sum of their counts -- packed as (group << 40) | count.  A count of 2^32 or more lowers the error word to
//                 the group (atomicMin: the lowest group wins).
//   k_ib_finish   one bisecting lane per group over the packed runs gives the CSR's offsets (a stretch of empty groups costs
//                 a lane each and nothing else); the counts are narrowed to the u32 abundances on the side.
//
// A thread of heads / emit holds 8 elements: step s of the workgroup takes elements [256 s, 256 s + 256) of the tile, wave w
// of it the 64 from 64 w on.  Nothing spins, no workgroup waits for another; the only atomic is the error word's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.hpp"

namespace smh {
namespace {

constexpr uint32_t kSteps = kBuildTile / kBuildThreads;   // 8
constexpr uint32_t kWaves = kBuildThreads / 64;           // 4
constexpr uint64_t kFixedGrid = 2048;                     // the grid limit of the launches that are given no device: groups, rebase
static_assert(kBuildTile % kBuildThreads == 0 && kBuildThreads % 64 == 0, "whole waves, whole steps");

// bit s: element tile * kBuildTile + s * kBuildThreads + tid is a head
__device__ __forceinline__ uint32_t heads_of(const uint64_t* __restrict__ hash, const uint64_t* __restrict__ tag, uint64_t n, int shift) {
  const uint64_t first = (uint64_t)blockIdx.x * kBuildTile + threadIdx.x;
  uint32_t mask = 0;
#pragma unroll
  for (uint32_t s = 0; s < kSteps; s++) {
    const uint64_t i = first + (uint64_t)s * kBuildThreads;
    if (i >= n) break;
    const bool head = i == 0 || hash[i] != hash[i - 1] || (tag[i] >> shift) != (tag[i - 1] >> shift);
    mask |= head ? 1u << s : 0u;
  }
  return mask;
}

__global__ __launch_bounds__(kBuildThreads) void k_ib_heads(const uint64_t* __restrict__ hash, const uint64_t* __restrict__ tag, uint64_t n,
                                                            int shift, uint32_t* __restrict__ tile_heads) {
  __shared__ uint32_t part[kWaves];
  const uint32_t mask = heads_of(hash, tag, n, shift);
  uint32_t k = 0;
#pragma unroll
  for (uint32_t s = 0; s < kSteps; s++) k += (uint32_t)__popcll(__ballot((mask >> s) & 1u));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
    for (uint32_t w = 0; w < kWaves; w++) sum += part[w];
    tile_heads[blockIdx.x] = sum;
  }
}

// tile_heads: scanned, tiles + 1 entries (the last: the total)
__global__ __launch_bounds__(kBuildThreads) void k_ib_emit(const uint64_t* __restrict__ hash, const uint64_t* __restrict__ tag, uint64_t n,
                                                           int shift, const uint32_t* __restrict__ tile_heads, uint64_t* __restrict__ run_hash,
                                                           uint32_t* __restrict__ run_start) {
  __shared__ uint32_t part[kSteps * kWaves];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t start = tile_heads[blockIdx.x];
  if (tile_heads[blockIdx.x + 1] == start) return;   // (uniform: a tile inside one run)
  const uint32_t mask = heads_of(hash, tag, n, shift);
  uint64_t votes[kSteps];
#pragma unroll
  for (uint32_t s = 0; s < kSteps; s++) {
    votes[s] = __ballot((mask >> s) & 1u);
    if (lane == 0) part[s * kWaves + wave] = (uint32_t)__popcll(votes[s]);
  }
  __syncthreads();
  const uint64_t below = (1ull << lane) - 1;
  const uint64_t first = (uint64_t)blockIdx.x * kBuildTile + threadIdx.x;
  uint32_t at = start;
  for (uint32_t w = 0; w < wave; w++) at += part[w];
#pragma unroll
  for (uint32_t s = 0; s < kSteps; s++) {
    if ((mask >> s) & 1u) {
      const uint64_t i = first + (uint64_t)s * kBuildThreads;
      const uint32_t r = at + (uint32_t)__popcll(votes[s] & below);
      run_hash[r] = hash[i];
      run_start[r] = (uint32_t)i;
    }
    // on to this wave's place in the next step: the rest of this step's waves, then the next step's waves in front of it
    if (s + 1 < kSteps) {
      for (uint32_t w = wave; w < kWaves; w++) at += part[s * kWaves + w];
      for (uint32_t w = 0; w < wave; w++) at += part[(s + 1) * kWaves + w];
    }
  }
}

__global__ __launch_bounds__(256) void k_ib_counts(const uint64_t* __restrict__ tag, uint64_t n, int shift, const uint32_t* __restrict__ run_start,
                                                   uint32_t nruns, uint64_t* __restrict__ run_pack, uint32_t* __restrict__ err) {
  const uint64_t low = (1ull << kBuildCountBits) - 1;
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < nruns; r += (uint64_t)gridDim.x * 256) {
    const uint64_t a = run_start[r], e = r + 1 < nruns ? (uint64_t)run_start[r + 1] : n;
    const uint64_t g = tag[a] >> shift;
    uint64_t c = e - a;
    if (shift) {
      c = 0;
      for (uint64_t k = a; k < e; k++) c += tag[k] & low;
    }
    if (c >> 32) atomicMin(err, (uint32_t)g);
    run_pack[r] = (g << kBuildCountBits) | (c & 0xffffffffull);
  }
}

__global__ __launch_bounds__(256) void k_ib_finish(const uint64_t* __restrict__ run_pack, uint32_t n_runs, uint32_t n_groups,
                                                   uint64_t* __restrict__ offsets, uint32_t* __restrict__ abunds) {
  const uint64_t step = (uint64_t)gridDim.x * 256, t0 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  for (uint64_t g = t0; g <= n_groups; g += step) {
    uint32_t lo = 0, hi = n_runs;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if ((run_pack[mid] >> kBuildCountBits) < g) lo = mid + 1; else hi = mid;
    }
    offsets[g] = lo;
  }
  if (abunds)
    for (uint64_t r = t0; r < n_runs; r += step) abunds[r] = (uint32_t)run_pack[r];
}

__global__ __launch_bounds__(256) void k_ib_groups(const uint32_t* __restrict__ groups, uint64_t n_entries, uint32_t per, uint32_t* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_entries; i += (uint64_t)gridDim.x * 256) {
    const uint64_t r = i / per;
    out[i] = groups ? groups[r] : (uint32_t)r;
  }
}

__global__ __launch_bounds__(256) void k_ib_rebase(const uint64_t* __restrict__ src, uint64_t n, uint64_t delta, uint64_t* __restrict__ dst) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) dst[i] = src[i] + delta;
}

}  // namespace

void index_build_geometry(uint32_t* tile_elems, uint32_t* threads) {
  if (tile_elems) *tile_elems = kBuildTile;
  if (threads) *threads = kBuildThreads;
}

void launch_index_build_groups(const uint32_t* groups, uint64_t n_entries, uint32_t per, uint32_t* out, hipStream_t s) {
  if (n_entries == 0) return;
  hipLaunchKernelGGL(k_ib_groups, dim3(grid_for(n_entries, 256, kFixedGrid, Device::get())), dim3(256), 0, s, groups, n_entries, per, out);
  HIP_CHECK(hipGetLastError());
}

void launch_index_build_heads(const uint64_t* hash, const uint64_t* tag, uint64_t n, int shift, uint32_t* tile_heads, Device& dev,
                              hipStream_t s) {
  if (n == 0) return;
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_ib_heads, dim3(index_build_tiles(n)), dim3(kBuildThreads), 0, s, hash, tag, n, shift, tile_heads);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("index_build_heads", s);
}

void launch_index_build_emit(const uint64_t* hash, const uint64_t* tag, uint64_t n, int shift, const uint32_t* tile_heads,
                             uint64_t* run_hash, uint32_t* run_start, Device& dev, hipStream_t s) {
  if (n == 0) return;
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_ib_emit, dim3(index_build_tiles(n)), dim3(kBuildThreads), 0, s, hash, tag, n, shift, tile_heads, run_hash, run_start);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("index_build_emit", s);
}

void launch_index_build_counts(const uint64_t* tag, uint64_t n, int shift, const uint32_t* run_start, uint32_t nruns, uint64_t* run_pack,
                               uint32_t* err, Device& dev, hipStream_t s) {
  if (nruns == 0) return;
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_ib_counts, dim3(grid_for(nruns, 256, dev.grid_limit(), dev)), dim3(256), 0, s, tag, n, shift, run_start, nruns, run_pack, err);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("index_build_emit", s);
}

void launch_index_build_finish(const uint64_t* run_pack, uint32_t n_runs, uint32_t n_groups, uint64_t* offsets, uint32_t* abunds, Device& dev,
                               hipStream_t s) {
  const uint64_t items = std::max<uint64_t>((uint64_t)n_groups + 1, abunds ? n_runs : 0);
  hipLaunchKernelGGL(k_ib_finish, dim3(grid_for(items, 256, dev.grid_limit(), dev)), dim3(256), 0, s, run_pack, n_runs, n_groups, offsets, abunds);
  HIP_CHECK(hipGetLastError());
}

void launch_index_build_rebase(const uint64_t* src, uint64_t n, uint64_t delta, uint64_t* dst, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_ib_rebase, dim3(grid_for(n, 256, kFixedGrid, Device::get())), dim3(256), 0, s, src, n, delta, dst);
  HIP_CHECK(hipGetLastError());
}

}  // namespace smh
