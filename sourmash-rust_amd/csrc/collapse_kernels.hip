// collapse_kernels.hip -- gfx950 kernels of collapsing a resident index by groups (include/sourmash_amd.h, "Collapsing an
// index by groups").  The hash directory holds, per rank r (a distinct hash of the index), the ascending list
// of the nodes that hold it; a fold of that list through group[] gives c_g(h) for every group with a member there, and the
// groups with c_g(h) >= need_g are the rank's survivors.  Two passes walk the lists the same way: the count pass leaves the
// survivors per rank, the emit pass writes (group << 32 | rank) and the abundance at the scanned positions.  The lengths of
// the groups are read off the partitioned keys afterwards (k_collapse_bounds: one binary search per group) -- a histogram
// kept by the count pass would be one atomic per survivor on as few addresses as there are groups.
// Owner lists are very uneven, so there are three regimes, told apart by the list's length L:
//
//   k_collapse_lane   L <= kCollapseLaneMax: the lane that holds the rank.  One scan of the list per distinct group, each
//                     finding the smallest group not yet handled and its count: no scratch, groups come out ascending.
//                     Longer lists are appended to one of two compacted lists (count pass only; the emit pass reads them).
//   k_collapse_wave   L <= kCollapseWaveMax: one wave.  The owners' groups go to the wave's LDS scratch; every lane takes
//                     one entry at a time and reads the whole scratch (all lanes the same address: a broadcast), counting
//                     the entries of its group and whether it is the first of them.  The first entries of surviving groups
//                     are numbered by a ballot.
//   k_collapse_long   anything longer: one workgroup.  The range of groups the list touches is found first; LDS counters
//                     (and u64 sums) over kCollapseGroupTile groups at a time are filled by a walk of the list with LDS
//                     atomics, then read for the survivors.  Exact for any number of owners in any number of groups.
//
// Inside a rank the survivors are written in whatever order the regime finds them: a group appears at most once per rank, so
// the stable partition by group that follows (sort.hip) leaves every group ascending by rank -- by hash -- either way, and
// the child is the same bytes.  Integer atomics only; no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "directory_probe.hpp"
#include "kernels.hpp"

namespace smh {
namespace {

// the abundance of hash h in node v: h's place in v's slice of the CSR (the directory keeps no positions)
__device__ __forceinline__ uint32_t abundance_of(const CollapseFold& f, uint32_t v, uint64_t h) {
  uint64_t lo = f.offsets[v], hi = f.offsets[v + 1];
  const uint64_t end = hi;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (f.hashes[mid] < h) lo = mid + 1; else hi = mid;
  }
  return lo < end && f.hashes[lo] == h ? f.abunds[lo] : 0u;
}

// one survivor at position `at`: group g holds rank r in c members whose abundances add up to sum
__device__ __forceinline__ void put(const CollapseFold& f, uint32_t at, uint32_t g, uint32_t r, uint32_t c, uint64_t sum) {
  f.key[at] = ((uint64_t)g << 32) | r;
  if (f.abund == kCollapseCount) f.val[at] = c;
  if (f.abund == kCollapseSum) {
    if (sum >> 32) atomicMin(f.err, g);
    f.val[at] = (uint32_t)sum;
  }
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_collapse_lane(CollapseFold f) {
  for (uint64_t r0 = (uint64_t)blockIdx.x * 256 + threadIdx.x; r0 < f.d.n_hashes; r0 += (uint64_t)gridDim.x * 256) {
    const uint32_t r = (uint32_t)r0;
    uint32_t b, e;
    directory_owner_range(f.d, r, &b, &e);
    if (e - b > kCollapseLaneMax) {
      if (!EMIT) {
        if (e - b > kCollapseWaveMax) f.long_list[atomicAdd(&f.list_count[1], 1u)] = r;
        else f.wave_list[atomicAdd(&f.list_count[0], 1u)] = r;
      }
      continue;
    }
    const uint32_t at = EMIT ? f.cnt[r] : 0u;
    uint32_t kept = 0;
    // groups >= from are still to be handled; kCollapseDrop is never one
    for (uint32_t from = 0;;) {
      uint32_t g = kCollapseDrop, c = 0;
      for (uint32_t k = b; k < e; k++) {
        const uint32_t x = f.group[f.d.owners[k]];
        if (x == kCollapseDrop || x < from) continue;
        if (x < g) { g = x; c = 1; } else if (x == g) c++;
      }
      if (g == kCollapseDrop) break;
      if (c >= f.need[g]) {
        if (EMIT) {
          uint64_t sum = 0;
          if (f.abund == kCollapseSum) {
            const uint64_t h = f.d.U[r];
            for (uint32_t k = b; k < e; k++) {
              const uint32_t v = f.d.owners[k];
              if (f.group[v] == g) sum += abundance_of(f, v, h);
            }
          }
          put(f, at + kept, g, r, c, sum);
        }
        kept++;
      }
      from = g + 1;   // (g < kCollapseDrop: no wrap; from == kCollapseDrop ends the next scan empty-handed)
    }
    if (!EMIT) f.cnt[r] = kept;
  }
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_collapse_wave(CollapseFold f) {
  __shared__ uint32_t scratch[4][kCollapseWaveMax];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = f.list_count[0];
  uint32_t* sg = scratch[w];
  for (uint32_t i0 = blockIdx.x * 4; i0 < n; i0 += gridDim.x * 4) {   // (uniform over the workgroup: the barriers below)
    const uint32_t i = i0 + w;
    const bool on = i < n;
    uint32_t r = 0, b = 0, e = 0;
    if (on) { r = f.wave_list[i]; directory_owner_range(f.d, r, &b, &e); }
    const uint32_t L = e - b;   // (uniform over the wave; at most kCollapseWaveMax: the lane kernel sorted the ranks)
    __syncthreads();            // the previous round's readers are done
    for (uint32_t k = lane; k < L; k += 64) sg[k] = f.group[f.d.owners[b + k]];
    __syncthreads();
    const uint32_t at = EMIT && on ? f.cnt[r] : 0u;
    uint32_t kept = 0;
    for (uint32_t j0 = 0; j0 < L; j0 += 64) {   // whole waves stay in the loop for the ballot
      const uint32_t j = j0 + lane;
      const uint32_t g = j < L ? sg[j] : kCollapseDrop;
      uint32_t c = 0;
      bool first = g != kCollapseDrop;
      for (uint32_t k = 0; k < L; k++) {
        const bool same = sg[k] == g;
        c += same ? 1u : 0u;
        first = first && !(same && k < j);
      }
      const bool surv = first && c >= f.need[g];
      const uint64_t m = __ballot(surv);
      if (EMIT && surv) {
        uint64_t sum = 0;
        if (f.abund == kCollapseSum) {
          const uint64_t h = f.d.U[r];
          for (uint32_t k = 0; k < L; k++)
            if (sg[k] == g) sum += abundance_of(f, f.d.owners[b + k], h);
        }
        put(f, at + kept + (uint32_t)__popcll(m & ((1ull << lane) - 1)), g, r, c, sum);
      }
      kept += (uint32_t)__popcll(m);
    }
    if (!EMIT && on && lane == 0) f.cnt[r] = kept;
  }
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_collapse_long(CollapseFold f) {
  __shared__ uint32_t sc[kCollapseGroupTile];
  __shared__ unsigned long long ss[kCollapseGroupTile];
  __shared__ uint32_t s_lo, s_hi, s_kept;
  const uint32_t tid = threadIdx.x, n = f.list_count[1];
  const bool sums = EMIT && f.abund == kCollapseSum;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {   // (everything below is uniform over the workgroup)
    const uint32_t r = f.long_list[i];
    uint32_t b, e;
    directory_owner_range(f.d, r, &b, &e);
    const uint64_t h = f.d.U[r];
    if (tid == 0) { s_lo = kCollapseDrop; s_hi = 0; s_kept = 0; }
    __syncthreads();
    // the range of groups the list touches: only its tiles are visited
    uint32_t lo = kCollapseDrop, hi = 0;
    for (uint32_t k = b + tid; k < e; k += 256) {
      const uint32_t g = f.group[f.d.owners[k]];
      if (g != kCollapseDrop) { lo = min(lo, g); hi = max(hi, g); }
    }
    if (lo != kCollapseDrop) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    __syncthreads();
    lo = s_lo; hi = s_hi;
    const uint32_t at = EMIT ? f.cnt[r] : 0u;
    if (lo != kCollapseDrop) {
      for (uint32_t base = lo - lo % kCollapseGroupTile;; base += kCollapseGroupTile) {
        for (uint32_t j = tid; j < kCollapseGroupTile; j += 256) { sc[j] = 0; if (sums) ss[j] = 0; }
        __syncthreads();
        for (uint32_t k = b + tid; k < e; k += 256) {
          const uint32_t v = f.d.owners[k];
          const uint32_t g = f.group[v];
          if (g == kCollapseDrop || g - base >= kCollapseGroupTile) continue;   // (g < base wraps to a large value)
          atomicAdd(&sc[g - base], 1u);
          if (sums) atomicAdd(&ss[g - base], (unsigned long long)abundance_of(f, v, h));
        }
        __syncthreads();
        for (uint32_t j = tid; j < kCollapseGroupTile; j += 256) {
          const uint32_t c = sc[j], g = base + j;
          if (c == 0 || g >= f.n_groups || c < f.need[g]) continue;
          const uint32_t p = atomicAdd(&s_kept, 1u);
          if (EMIT) put(f, at + p, g, r, c, sums ? ss[j] : 0ull);
        }
        __syncthreads();
        if (hi - base < kCollapseGroupTile) break;   // (base <= lo <= hi; left before base could wrap)
      }
    }
    if (!EMIT && tid == 0) f.cnt[r] = s_kept;
    __syncthreads();   // s_kept is reset by the next rank
  }
}

// key: the survivors partitioned by group
__global__ __launch_bounds__(256) void k_collapse_finish(const uint64_t* __restrict__ U, const uint64_t* __restrict__ key,
                                                         const uint32_t* __restrict__ val, uint32_t S, uint64_t* __restrict__ out_hashes,
                                                         uint32_t* __restrict__ out_abunds) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < S; i += (uint64_t)gridDim.x * 256) {
    out_hashes[i] = U[(uint32_t)key[i]];
    if (out_abunds) out_abunds[i] = val[i];
  }
}

// key: the survivors partitioned by group; start[g] = the survivors of the groups below g, for g = 0 .. G
__global__ __launch_bounds__(256) void k_collapse_bounds(const uint64_t* __restrict__ key, uint32_t S, uint32_t G, uint32_t* __restrict__ start) {
  for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g <= G; g += (uint64_t)gridDim.x * 256) {
    const uint64_t first = g << 32;   // the smallest key of group g
    uint32_t lo = 0, hi = S;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (key[mid] < first) lo = mid + 1; else hi = mid;
    }
    start[g] = lo;
  }
}


template <bool EMIT>
void launch_fold(const CollapseFold& f, Device& dev, hipStream_t s) {
  // (the long lists number at most n_pairs / (their shortest length): the grids are sized for that, the kernels read the counts)
  hipLaunchKernelGGL(k_collapse_lane<EMIT>, dim3(grid_for(f.d.n_hashes, 256, dev.grid_limit(), dev)), dim3(256), 0, s, f);
  hipLaunchKernelGGL(k_collapse_wave<EMIT>, dim3(grid_for(f.d.n_pairs / (kCollapseLaneMax + 1) + 1, 4, dev.grid_limit(), dev)), dim3(256), 0, s, f);
  hipLaunchKernelGGL(k_collapse_long<EMIT>, dim3(grid_for(f.d.n_pairs / (kCollapseWaveMax + 1) + 1, 1, dev.grid_limit(), dev)), dim3(256), 0, s, f);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

void collapse_geometry(uint32_t* lane_max, uint32_t* wave_max, uint32_t* group_tile) {
  if (lane_max) *lane_max = kCollapseLaneMax;
  if (wave_max) *wave_max = kCollapseWaveMax;
  if (group_tile) *group_tile = kCollapseGroupTile;
}

void launch_collapse_count(const CollapseFold& f, Device& dev, hipStream_t s) {
  if (f.d.n_hashes == 0) return;
  dev.prof_begin(s);
  HIP_CHECK(hipMemsetAsync(f.list_count, 0, 8, s));
  launch_fold<false>(f, dev, s);
  dev.prof_end("collapse_count", s);
}

void launch_collapse_emit(const CollapseFold& f, Device& dev, hipStream_t s) {
  if (f.d.n_hashes == 0) return;
  dev.prof_begin(s);
  launch_fold<true>(f, dev, s);
  dev.prof_end("collapse_emit", s);
}

void launch_collapse_bounds(const uint64_t* key, uint32_t S, uint32_t n_groups, uint32_t* start, Device& dev, hipStream_t s) {
  hipLaunchKernelGGL(k_collapse_bounds, dim3(grid_for((uint64_t)n_groups + 1, 256, dev.grid_limit(), dev)), dim3(256), 0, s, key, S, n_groups, start);
  HIP_CHECK(hipGetLastError());
}

void launch_collapse_finish(const uint64_t* U, const uint64_t* key, const uint32_t* val, uint32_t S, uint64_t* out_hashes,
                            uint32_t* out_abunds, Device& dev, hipStream_t s) {
  if (S == 0) return;
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_collapse_finish, dim3(grid_for(S, 256, dev.grid_limit(), dev)), dim3(256), 0, s, U, key, val, S, out_hashes, out_abunds);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("collapse_finish", s);
}

}  // namespace smh
