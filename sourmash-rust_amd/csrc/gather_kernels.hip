// gather_kernels.hip -- gfx950 kernels of gather: the greedy decomposition of one query against a resident index
// (include/sourmash_amd.h, smh_index_gather).  Round r reports the sketch that holds the most of what is
// still unexplained in the query -- the lowest index on ties -- and removes its hashes from the query.
//
// The expensive part is done ONCE per call:
//   k_gather_hits      one wavefront per resident sketch streams it 64 elements per step (as wave_pair of
//                      compare_kernels.hip does) and looks every element up in the query Q.  Q does not fit LDS when it
//                      matters (a metagenome: 10^5 .. 10^6 hashes), so LDS holds a sampled top of it -- every 2^s-th hash,
//                      at most kGatherSamples of them -- and the last s levels of the search read global memory.  The
//                      lower end of the search window is carried from step to step (elements ascend).  Per sketch: the
//                      query positions it holds, compacted by the ballot prefix (the hit list), their number c0 (the
//                      round counters start there), and per query position its degree.
//   (scan of the degrees: exclusive_scan_u32_dev)
//   k_gather_invert    the inverted lists, query position -> sketches that hold it (order inside a list is free).
// A round is then two small launches and no host work:
//   k_gather_pick      arg-max of the n counters, lowest index on ties: max of (c << 32) | ~i.  Writes the row, or raises
//                      the device-side `done` word when the best count is below the threshold or the rows are full.
//   k_gather_subtract  walks the winner's hit list, labels the positions nobody consumed yet, sums their abundances into
//                      the row and decrements the counter of every sketch in each position's inverted list.  Integer
//                      atomics: the result does not depend on the order.  Lists longer than kGatherShortList are walked
//                      by the whole wave.
// Both read `best` and `done` from device memory and return at once when `done` is set, so the host queues
// kGatherRoundsPerSync rounds between two 8-byte read-backs.  No cooperative launch, no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.hpp"
#include "wave_ops.hpp"

namespace smh {
namespace {

constexpr uint32_t kGatherSamples = 4096;   // sampled top of the query: 32 KiB of LDS per workgroup
constexpr uint32_t kGatherShortList = 8;    // inverted lists up to this length are walked by the lane that consumed the position
constexpr uint32_t kUnassigned = 0xffffffffu;

struct GatherState {
  uint32_t done;     // raised by k_gather_pick: nothing reaches the threshold, or the rows are full
  uint32_t rounds;   // rows written
  uint32_t best;     // the winner of the running round
  uint32_t pad;
  unsigned long long total_hits;
};

// m = ceil(lq / 2^shift) <= kGatherSamples samples; shift == 0: the whole query sits in LDS and no global level is left
__global__ __launch_bounds__(256) void k_gather_hits(SketchSet idx, const uint64_t* __restrict__ Q, uint32_t lq, uint32_t shift,
                                                     uint32_t m, uint32_t* __restrict__ hits, uint32_t* __restrict__ c0,
                                                     uint32_t* __restrict__ c, uint32_t* __restrict__ deg, GatherState* st) {
  __shared__ uint64_t samp[kGatherSamples];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (uint32_t t = tid; t < m; t += 256) samp[t] = Q[(uint64_t)t << shift];
  __syncthreads();
  for (uint32_t node = blockIdx.x * 4 + w; node < idx.n; node += gridDim.x * 4) {
    const uint64_t ao = idx.offsets[node];
    const uint32_t la = (uint32_t)(idx.offsets[node + 1] - ao);
    const uint64_t* __restrict__ A = idx.hashes + ao;
    uint32_t* __restrict__ H = hits + ao;
    uint32_t base = 0, cc = 0;   // base: every Q[< base] is smaller than this step's elements
    for (uint32_t i0 = 0; i0 < la; i0 += 64) {
      const uint32_t i = i0 + lane;
      const bool ok = i < la;
      const uint64_t a = ok ? A[i] : ~0ull;
      // js = number of samples below a; the samples in front of ceil(base / 2^s) are known to be
      uint32_t lo = (uint32_t)(((uint64_t)base + (1ull << shift) - 1) >> shift), len = m - lo;
      while (len > 0) {
        const uint32_t half = len >> 1, mid = lo + half;
        const bool lt = samp[mid] < a;
        lo = lt ? mid + 1 : lo;
        len = lt ? len - half - 1 : half;
      }
      // sample js - 1 < a <= sample js: the lower bound lies in ((js - 1) << s, js << s], and not below base
      uint32_t g = 0;
      if (lo != 0) {
        const uint32_t wlo = max(((lo - 1) << shift) + 1, base);
        const uint32_t whi = (uint32_t)min((uint64_t)lo << shift, (uint64_t)lq);
        g = wlo; len = whi - wlo;
        while (len > 0) {
          const uint32_t half = len >> 1, mid = g + half;
          const bool lt = Q[mid] < a;
          g = lt ? mid + 1 : g;
          len = lt ? len - half - 1 : half;
        }
      }
      const bool match = ok && g < lq && Q[g] == a;
      const uint64_t mm = __ballot(match);
      if (match) {
        H[cc + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull))] = g;
        atomicAdd(&deg[g], 1u);
      }
      cc += (uint32_t)__popcll(mm);
      base = (uint32_t)__builtin_amdgcn_readlane((int)g, 63);
    }
    if (lane == 0) {
      c0[node] = cc;
      c[node] = cc;
      if (cc) atomicAdd(&st->total_hits, (unsigned long long)cc);
    }
  }
}

// inv_off: exclusive scan of the degrees (lq + 1 entries); cursor: zeroed, one counter per query position
__global__ __launch_bounds__(256) void k_gather_invert(SketchSet idx, const uint32_t* __restrict__ hits, const uint32_t* __restrict__ c0,
                                                       const uint32_t* __restrict__ inv_off, uint32_t* __restrict__ cursor,
                                                       uint32_t* __restrict__ inv) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint32_t node = blockIdx.x * 4 + w; node < idx.n; node += gridDim.x * 4) {
    const uint32_t* __restrict__ H = hits + idx.offsets[node];
    const uint32_t cnt = c0[node];
    for (uint32_t k = lane; k < cnt; k += 64) {
      const uint32_t p = H[k];
      inv[inv_off[p] + atomicAdd(&cursor[p], 1u)] = node;
    }
  }
}

// one workgroup; lens: the sketches' CSR offsets (size_match)
__global__ __launch_bounds__(1024) void k_gather_pick(const uint32_t* __restrict__ c, uint32_t n, const uint32_t* __restrict__ c0,
                                                      const uint64_t* __restrict__ offsets, uint32_t threshold, uint32_t capacity,
                                                      GatherRow* __restrict__ rows, GatherState* st) {
  __shared__ uint64_t part[16];
  if (st->done) return;
  uint64_t best = 0;
  for (uint32_t i = threadIdx.x; i < n; i += 1024) {
    const uint64_t key = ((uint64_t)c[i] << 32) | (uint32_t)~i;
    best = key > best ? key : best;
  }
  best = wave_max_u64(best);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (uint32_t k = 1; k < 16; k++) best = part[k] > best ? part[k] : best;
  const uint32_t cbest = (uint32_t)(best >> 32), i = ~(uint32_t)best, r = st->rounds;
  if (cbest < threshold || r == capacity) { st->done = 1; return; }
  GatherRow row;
  row.match = i; row.common_remaining = cbest; row.common_original = c0[i];
  row.size_match = (uint32_t)(offsets[i + 1] - offsets[i]); row.abund_sum = 0;
  rows[r] = row;
  st->best = i;
  st->rounds = r + 1;
}

// abundance of query position p: u64 counts, or run starts (the last run ends at `total`), or 1
struct GatherWeights { const uint64_t* counts; const uint32_t* starts; uint32_t total; };

__global__ __launch_bounds__(256) void k_gather_subtract(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ hits,
                                                         const uint32_t* __restrict__ c0, const uint32_t* __restrict__ inv_off,
                                                         const uint32_t* __restrict__ inv, uint32_t lq, GatherWeights wt,
                                                         uint32_t* __restrict__ c, uint32_t* __restrict__ assigned,
                                                         GatherRow* __restrict__ rows, const GatherState* st) {
  if (st->done) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t node = st->best, r = st->rounds - 1;
  const uint32_t* __restrict__ H = hits + offsets[node];
  const uint32_t L = c0[node];
  const uint32_t nw = gridDim.x * 4;
  uint64_t wsum = 0;
  for (uint32_t k0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; k0 < L; k0 += nw * 64) {
    const uint32_t k = k0 + lane;
    bool take = false;
    uint32_t b = 0, e = 0;
    if (k < L) {
      const uint32_t p = H[k];
      if (assigned[p] == kUnassigned) {   // a position sits once in a hit list: no other lane looks at this word
        take = true;
        assigned[p] = r;
        wsum += wt.counts ? wt.counts[p] : wt.starts ? (uint64_t)((p + 1 < lq ? wt.starts[p + 1] : wt.total) - wt.starts[p]) : 1ull;
        b = inv_off[p]; e = inv_off[p + 1];
      }
    }
    const bool longl = take && e - b > kGatherShortList;
    if (take && !longl)
      for (uint32_t t = b; t < e; t++) atomicSub(&c[inv[t]], 1u);
    uint64_t lm = __ballot(longl);
    while (lm) {
      const int src = __builtin_ctzll(lm);
      lm &= lm - 1;
      const uint32_t bb = (uint32_t)__shfl((int)b, src), ee = (uint32_t)__shfl((int)e, src);
      for (uint32_t t = bb + lane; t < ee; t += 64) atomicSub(&c[inv[t]], 1u);
    }
  }
  wsum = wave_sum_u64(wsum);
  if (lane == 0 && wsum) atomicAdd((unsigned long long*)&rows[r].abund_sum, (unsigned long long)wsum);
}

}  // namespace

uint32_t gather_run(const SketchSet& idx, uint32_t max_len, const GatherQuery& q, uint32_t threshold, GatherRow* rows_host,
                    uint32_t capacity, uint32_t* assigned_host, Device& dev, hipStream_t s) {
  const uint32_t n = idx.n, lq = q.n;
  const uint64_t n_elems = idx.h_offsets[n] - idx.h_offsets[0];
  if (threshold == 0) threshold = 1;
  // a round empties at least the winner's counter, so there are at most n of them
  const uint32_t cap = std::min(capacity, n);
  uint32_t shift = 0;
  while ((((uint64_t)lq + (1ull << shift) - 1) >> shift) > kGatherSamples) shift++;
  const uint32_t m = (uint32_t)(((uint64_t)lq + (1ull << shift) - 1) >> shift);

  Workspace ws(s);
  uint32_t* hits = ws.take<uint32_t>(n_elems);
  uint32_t* d_c0 = ws.take<uint32_t>((size_t)n * 2);
  uint32_t* d_c = d_c0 + n;
  uint32_t* d_invoff = ws.take<uint32_t>((size_t)lq * 3 + 1);   // lq + 1: degrees, then their exclusive scan
  uint32_t* d_cursor = d_invoff + lq + 1;            // lq
  uint32_t* d_assigned = d_cursor + lq;              // lq
  GatherRow* rows = ws.take<GatherRow>(std::max(cap, 1u));
  GatherState* d_st = ws.take<GatherState>(1);
  HIP_CHECK(hipMemsetAsync(d_invoff, 0, ((size_t)lq + 1) * 4 + (size_t)lq * 4, s));
  HIP_CHECK(hipMemsetAsync(d_assigned, 0xff, (size_t)lq * 4, s));
  HIP_CHECK(hipMemsetAsync(d_st, 0, sizeof(GatherState), s));

  const uint32_t grid = grid_for(n, 4, dev.grid_limit(), dev);
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_gather_hits, dim3(grid), dim3(256), 0, s, idx, q.hashes, lq, shift, m, hits, d_c0, d_c, d_invoff, d_st);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("gather_hits", s);
  GatherState h_st;
  HIP_CHECK(hipMemcpyAsync(&h_st, d_st, sizeof h_st, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (h_st.total_hits >= (1ull << 32)) throw_internal("gather: 2^32 or more (sketch, query hash) matches in one call");
  const uint32_t total_hits = (uint32_t)h_st.total_hits;

  uint32_t rounds = 0;
  uint32_t* inv = ws.take<uint32_t>(std::max(total_hits, 1u));
  if (total_hits != 0 && cap != 0) {
    dev.prof_begin(s);
    exclusive_scan_u32_dev(d_invoff, (size_t)lq + 1, nullptr, dev.scratch, s);
    hipLaunchKernelGGL(k_gather_invert, dim3(grid), dim3(256), 0, s, idx, hits, d_c0, d_invoff, d_cursor, inv);
    HIP_CHECK(hipGetLastError());
    dev.prof_end("gather_invert", s);
    const GatherWeights wt{q.counts, q.starts, q.total};
    const uint32_t sub_grid = grid_for(std::min(max_len, lq), 256, 256, dev);
    for (;;) {
      dev.prof_begin(s);
      for (uint32_t k = 0; k < kGatherRoundsPerSync; k++) {
        hipLaunchKernelGGL(k_gather_pick, dim3(1), dim3(1024), 0, s, d_c, n, d_c0, idx.offsets, threshold, cap, rows, d_st);
        hipLaunchKernelGGL(k_gather_subtract, dim3(sub_grid), dim3(256), 0, s, idx.offsets, hits, d_c0, d_invoff,
                           inv, lq, wt, d_c, d_assigned, rows, d_st);
      }
      HIP_CHECK(hipGetLastError());
      dev.prof_end("gather_rounds", s);
      HIP_CHECK(hipMemcpyAsync(&h_st, d_st, 8, hipMemcpyDeviceToHost, s));   // {done, rounds}
      HIP_CHECK(hipStreamSynchronize(s));
      if (h_st.done || h_st.rounds >= cap) break;
    }
    rounds = h_st.rounds;
  }
  if (rounds) HIP_CHECK(hipMemcpyAsync(rows_host, rows, (size_t)rounds * sizeof(GatherRow), hipMemcpyDeviceToHost, s));
  if (assigned_host && lq) HIP_CHECK(hipMemcpyAsync(assigned_host, d_assigned, (size_t)lq * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return rounds;
}

}  // namespace smh
