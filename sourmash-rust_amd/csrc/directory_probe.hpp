// directory_probe.hpp -- device code shared by the kernels that look hashes up in an index's hash directory
// (match_kernels.hip, gather_many_kernels.hip, search_many_kernels.hip; MatchDirectory is in kernels.hpp).  U, the sorted distinct hashes of the whole
// index, does not fit LDS when it matters, so LDS holds its sampled top -- every 2^s-th hash, at most kMatchSamples -- and
// the last s levels of the search read global memory inside a window of 2^s (as k_gather_hits searches the query).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace smh {

// m = ceil(n_hashes / 2^shift) <= kMatchSamples samples; shift == 0: all of U sits in LDS and no global level is left
inline void directory_sampling(uint32_t n_hashes, uint32_t* shift, uint32_t* m) {
  uint32_t sh = 0;
  while ((((uint64_t)n_hashes + (1ull << sh) - 1) >> sh) > kMatchSamples) sh++;
  *shift = sh;
  *m = (uint32_t)(((uint64_t)n_hashes + (1ull << sh) - 1) >> sh);
}

// owners of rank g: d.owners[b .. e)
__device__ __forceinline__ void directory_owner_range(const MatchDirectory& d, uint32_t g, uint32_t* b, uint32_t* e) {
  *b = d.starts[g];
  *e = g + 1 < d.n_hashes ? d.starts[g + 1] : d.n_pairs;
}

// the workgroup's copy of the sampled top (samp: kMatchSamples entries of LDS); every thread of the workgroup calls it
__device__ __forceinline__ void directory_stage_samples(const MatchDirectory& d, uint32_t shift, uint32_t m, uint64_t* samp) {
  for (uint32_t t = threadIdx.x; t < m; t += blockDim.x) samp[t] = d.U[(uint64_t)t << shift];
  __syncthreads();
}

// the number of hashes of U below h (the rank of h when U holds it); a lane with !ok searches nothing and gets 0
__device__ __forceinline__ uint32_t directory_lower_bound(const MatchDirectory& d, const uint64_t* samp, uint32_t shift, uint32_t m,
                                                          uint64_t h, bool ok) {
  // js = number of samples below h
  uint32_t lo = 0, len = ok ? m : 0;
  while (len > 0) {
    const uint32_t half = len >> 1, mid = lo + half;
    const bool lt = samp[mid] < h;
    lo = lt ? mid + 1 : lo;
    len = lt ? len - half - 1 : half;
  }
  // sample js - 1 < h <= sample js: the lower bound lies in ((js - 1) << s, js << s]
  uint32_t g = 0;
  if (lo != 0) {
    const uint32_t wlo = ((lo - 1) << shift) + 1;
    const uint32_t whi = (uint32_t)min((uint64_t)lo << shift, (uint64_t)d.n_hashes);
    g = wlo; len = whi - wlo;
    while (len > 0) {
      const uint32_t half = len >> 1, mid = g + half;
      const bool lt = d.U[mid] < h;
      g = lt ? mid + 1 : g;
      len = lt ? len - half - 1 : half;
    }
  }
  return g;
}

// --- a chunk of queries probed at once (gather_many_kernels.hip, search_many_kernels.hip): position t of the chunk belongs to
// query q when qoff[q] <= t < qoff[q + 1], and every owner of a hit position is visited
constexpr uint32_t kShortOwners = 8;   // owner lists up to this length are walked by the lane that holds the position

// the query holding position t: the last q with qoff[q] <= t (empty queries share their start with the next one)
__device__ __forceinline__ uint32_t query_of(const uint32_t* __restrict__ qoff, uint32_t nq, uint32_t t) {
  uint32_t lo = 0, hi = nq;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (qoff[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// f(owner, q, t) for every owner in owners[b .. e) of every lane with `active`.  EVERY lane of the wave calls it: the long
// lists are handed round by ballot and walked by all 64 lanes.
template <class F>
__device__ __forceinline__ void walk_owners(const uint32_t* __restrict__ owners, bool active, uint32_t b, uint32_t e, uint32_t q,
                                            uint32_t t, uint32_t lane, F f) {
  const bool longl = active && e - b > kShortOwners;
  if (active && !longl)
    for (uint32_t k = b; k < e; k++) f(owners[k], q, t);
  uint64_t lm = __ballot(longl);
  while (lm) {
    const int src = __builtin_ctzll(lm);
    lm &= lm - 1;
    const uint32_t bb = (uint32_t)__shfl((int)b, src), ee = (uint32_t)__shfl((int)e, src);
    const uint32_t qq = (uint32_t)__shfl((int)q, src), tt = (uint32_t)__shfl((int)t, src);
    for (uint32_t k = bb + lane; k < ee; k += 64) f(owners[k], qq, tt);
  }
}

}  // namespace smh
