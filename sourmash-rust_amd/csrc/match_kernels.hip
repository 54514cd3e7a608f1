// match_kernels.hip -- gfx950 kernels of matching records against a resident index (include/sourmash_amd.h, "Matching
// records").  The grouped fold (sort.hip) has turned a batch into runs: one per distinct (record, hash),
// ordered by record, then hash.  Here every run is looked up in the index and every record is given its best node.
//
//   k_match_owner_ids    directory build: the node id of every element of the index's CSR (the payload of the stable sort
//                        that makes the inverted lists; the elements are in node order, so owners come out ascending)
//   k_match_probe        one lane per run: its rank in U, the sorted distinct hashes of the whole index, or a miss.  U does
//                        not fit LDS when it matters, so LDS holds its sampled top -- every 2^s-th hash, at most
//                        kMatchSamples -- and the last s levels of the search read global memory (as k_gather_hits).  The
//                        runs of one record are neighbours, so the four row sums, the record's owner-pair count and its
//                        first run are reduced over the wave by a segmented scan: one atomic per (record, wave).
//   k_match_tally        one wave per record.  A record whose owner pairs (hit runs x their owners) number at most
//                        kMatchLdsPairs copies the owners into its slice of LDS and counts there: every lane counts the
//                        copies of its elements, the wave takes the max of (count << 32 | ~node): the lowest node on ties.
//                        A record with more pairs is appended to the list of the dense regime.
//   k_match_dense_count  dense regime, a round of records: a slab of n_nodes counters per record in global memory, the
//   k_match_dense_pick   owners of the hit runs counted with integer atomics (short lists by the lane that holds the run,
//                        long ones by the whole wave), then one workgroup per record takes the arg-max.
//   k_match_hit_scatter  the optional hit list: the hashes of the hit runs, compacted in run order.
// Every count is an integer and every reduction is a sum or a max: no result depends on the order of the atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "directory_probe.hpp"
#include "kernels.hpp"
#include "wave_ops.hpp"

namespace smh {
namespace {

constexpr uint32_t kShortOwners = 8;   // owner lists up to this length are walked by the lane that holds the run

__global__ __launch_bounds__(256) void k_match_owner_ids(const uint64_t* __restrict__ offsets, uint32_t n, uint64_t total,
                                                         uint32_t* __restrict__ ids) {
  const uint64_t base = offsets[0];
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
    uint32_t lo = 0, hi = n;   // offsets[lo] <= base + t < offsets[hi]
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (offsets[mid] <= base + t) lo = mid; else hi = mid;
    }
    ids[t] = lo;
  }
}

// shift, m: directory_sampling (the search itself is directory_probe.hpp's, shared with gather_many_kernels.hip)
__global__ __launch_bounds__(256) void k_match_probe(MatchDirectory d, uint32_t shift, uint32_t m, const uint64_t* __restrict__ run_hash,
                                                     const uint64_t* __restrict__ run_rec, const uint32_t* __restrict__ run_start,
                                                     uint32_t nruns, uint32_t ncand, uint32_t rec0, MatchRow* __restrict__ rows,
                                                     uint32_t* __restrict__ rec_first, unsigned long long* __restrict__ rec_pairs,
                                                     uint32_t* __restrict__ rank_out, uint32_t* __restrict__ hit_flag) {
  __shared__ uint64_t samp[kMatchSamples];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  directory_stage_samples(d, shift, m, samp);
  const uint32_t nU = d.n_hashes;
  for (uint64_t i0 = (uint64_t)blockIdx.x * 256; i0 < nruns; i0 += (uint64_t)gridDim.x * 256) {
    const uint32_t i = (uint32_t)i0 + tid;   // (whole waves stay in the loop: the shuffles below see every lane)
    const bool ok = i < nruns;
    const uint64_t h = ok ? run_hash[i] : 0;
    const uint32_t g = directory_lower_bound(d, samp, shift, m, h, ok);
    const bool hit = ok && g < nU && d.U[g] == h;
    uint32_t deg = 0;
    if (hit) { uint32_t b, e; directory_owner_range(d, g, &b, &e); deg = e - b; }
    if (ok) {
      rank_out[i] = hit ? g : kMatchMiss;
      if (hit_flag) hit_flag[i] = hit ? 1u : 0u;
    }
    // the record's sums over the wave: inclusive segmented scan, the segments are the records (lanes past the end: their own)
    const uint32_t rec = ok ? (uint32_t)run_rec[i] - rec0 : 0xffffffffu;
    const uint32_t wl = ok ? (i + 1 < nruns ? run_start[i + 1] : ncand) - run_start[i] : 0;
    uint32_t s_w = wl, s_d = ok ? 1u : 0u, s_hw = hit ? wl : 0u, s_hd = hit ? 1u : 0u;
    uint64_t s_p = deg;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o_rec = __shfl_up(rec, off);
      const uint32_t o_w = __shfl_up(s_w, off), o_d = __shfl_up(s_d, off), o_hw = __shfl_up(s_hw, off), o_hd = __shfl_up(s_hd, off);
      const uint64_t o_p = __shfl_up(s_p, off);
      if (lane >= (uint32_t)off && o_rec == rec) { s_w += o_w; s_d += o_d; s_hw += o_hw; s_hd += o_hd; s_p += o_p; }
    }
    const uint32_t prev_rec = __shfl_up(rec, 1), next_rec = __shfl_down(rec, 1);
    if (ok && (lane == 0 || prev_rec != rec)) atomicMin(&rec_first[rec], i);
    if (ok && (lane == 63 || next_rec != rec)) {
      MatchRow* row = rows + rec;
      atomicAdd(&row->windows, s_w);
      atomicAdd(&row->distinct, s_d);
      if (s_hd) {
        atomicAdd(&row->hit_windows, s_hw);
        atomicAdd(&row->hit_distinct, s_hd);
        atomicAdd(&rec_pairs[rec], (unsigned long long)s_p);
      }
    }
  }
}

// rows, rec_first, rec_pairs: of the fold's nrec records, as k_match_probe left them
__global__ __launch_bounds__(256) void k_match_tally(MatchDirectory d, const uint32_t* __restrict__ rank, MatchRow* __restrict__ rows,
                                                     const uint32_t* __restrict__ rec_first,
                                                     const unsigned long long* __restrict__ rec_pairs, uint32_t nrec,
                                                     uint32_t* __restrict__ big_list, uint32_t* __restrict__ big_count) {
  __shared__ uint32_t own_all[4][kMatchLdsPairs];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t* own = own_all[w];
  for (uint32_t r = blockIdx.x * 4 + w; r < nrec; r += gridDim.x * 4) {   // (r is the wave's: every branch on it is uniform)
    const uint32_t hd = rows[r].hit_distinct;
    if (hd == 0) {
      if (lane == 0) { rows[r].best = kMatchMiss; rows[r].best_common = 0; }
      continue;
    }
    const uint64_t P = rec_pairs[r];
    if (P > kMatchLdsPairs) {
      if (lane == 0) big_list[atomicAdd(big_count, 1u)] = r;
      continue;
    }
    const uint32_t first = rec_first[r], cnt = rows[r].distinct;
    uint32_t fill = 0;
    for (uint32_t k0 = 0; k0 < cnt; k0 += 64) {
      const uint32_t k = k0 + lane;
      const uint32_t g = k < cnt ? rank[first + k] : kMatchMiss;
      uint32_t b = 0, e = 0;
      if (g != kMatchMiss) directory_owner_range(d, g, &b, &e);
      const uint32_t deg = e - b;
      uint32_t incl = deg;
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off);
        if (lane >= (uint32_t)off) incl += o;
      }
      const uint32_t at = fill + incl - deg;
      for (uint32_t t = 0; t < deg; t++) own[at + t] = d.owners[b + t];   // (at + deg <= P <= kMatchLdsPairs)
      fill += (uint32_t)__shfl((int)incl, 63);
    }
    // the lanes read what other lanes of the wave wrote
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    uint64_t best = 0;
    for (uint32_t e = lane; e < fill; e += 64) {
      const uint32_t v = own[e];
      uint32_t c = 0;
      for (uint32_t j = 0; j < fill; j++) c += own[j] == v ? 1u : 0u;
      const uint64_t key = ((uint64_t)c << 32) | (uint32_t)~v;
      best = key > best ? key : best;
    }
    best = wave_max_u64(best);
    if (lane == 0) { rows[r].best = ~(uint32_t)best; rows[r].best_common = (uint32_t)(best >> 32); }
    // the next record's writes stay behind these reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// round of `nbig` records (big[slot]), blocks_per_rec workgroups each; slab: nbig x n_nodes zeroed counters
__global__ __launch_bounds__(256) void k_match_dense_count(MatchDirectory d, const uint32_t* __restrict__ rank,
                                                           const MatchRow* __restrict__ rows, const uint32_t* __restrict__ rec_first,
                                                           const uint32_t* __restrict__ big, uint32_t blocks_per_rec, uint32_t n_nodes,
                                                           uint32_t* __restrict__ slab) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t slot = blockIdx.x / blocks_per_rec, part = blockIdx.x % blocks_per_rec;
  const uint32_t r = big[slot];
  uint32_t* __restrict__ c = slab + (size_t)slot * n_nodes;
  const uint32_t first = rec_first[r], cnt = rows[r].distinct;
  const uint32_t nw = blocks_per_rec * 4;
  for (uint64_t k0 = (uint64_t)(part * 4 + (threadIdx.x >> 6)) * 64; k0 < cnt; k0 += (uint64_t)nw * 64) {
    const uint32_t k = (uint32_t)k0 + lane;
    const uint32_t g = k < cnt ? rank[first + k] : kMatchMiss;
    uint32_t b = 0, e = 0;
    if (g != kMatchMiss) directory_owner_range(d, g, &b, &e);
    const bool longl = e - b > kShortOwners;
    if (!longl)
      for (uint32_t t = b; t < e; t++) atomicAdd(&c[d.owners[t]], 1u);
    uint64_t lm = __ballot(longl);
    while (lm) {
      const int src = __builtin_ctzll(lm);
      lm &= lm - 1;
      const uint32_t bb = (uint32_t)__shfl((int)b, src), ee = (uint32_t)__shfl((int)e, src);
      for (uint32_t t = bb + lane; t < ee; t += 64) atomicAdd(&c[d.owners[t]], 1u);
    }
  }
}

__global__ __launch_bounds__(256) void k_match_dense_pick(const uint32_t* __restrict__ slab, uint32_t n_nodes,
                                                          const uint32_t* __restrict__ big, MatchRow* __restrict__ rows) {
  __shared__ uint64_t part[4];
  const uint32_t* __restrict__ c = slab + (size_t)blockIdx.x * n_nodes;
  uint64_t best = 0;
  for (uint32_t i = threadIdx.x; i < n_nodes; i += 256) {
    const uint64_t key = ((uint64_t)c[i] << 32) | (uint32_t)~i;
    best = key > best ? key : best;
  }
  best = wave_max_u64(best);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (uint32_t k = 1; k < 4; k++) best = part[k] > best ? part[k] : best;
  MatchRow* row = rows + big[blockIdx.x];
  row->best = ~(uint32_t)best;
  row->best_common = (uint32_t)(best >> 32);
}

// at: the exclusive scan of the hit flags
__global__ __launch_bounds__(256) void k_match_hit_scatter(const uint64_t* __restrict__ run_hash, const uint32_t* __restrict__ rank,
                                                           const uint32_t* __restrict__ at, uint32_t nruns, uint64_t* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nruns; i += (uint64_t)gridDim.x * 256)
    if (rank[i] != kMatchMiss) out[at[i]] = run_hash[i];
}


}  // namespace

void match_geometry(uint32_t* lds_pairs, uint32_t* threads_per_record, uint32_t* probe_samples) {
  if (lds_pairs) *lds_pairs = kMatchLdsPairs;
  if (threads_per_record) *threads_per_record = kMatchThreadsPerRecord;
  if (probe_samples) *probe_samples = kMatchSamples;
}

void launch_match_owner_ids(const uint64_t* offsets_dev, uint32_t n, uint64_t total, uint32_t* ids, Device& dev, hipStream_t s) {
  if (total == 0) return;
  hipLaunchKernelGGL(k_match_owner_ids, dim3(grid_for(total, 256, dev.grid_limit(), dev)), dim3(256), 0, s, offsets_dev, n, total, ids);
  HIP_CHECK(hipGetLastError());
}

void launch_match_probe(const MatchDirectory& d, const uint64_t* run_hash, const uint64_t* run_rec, const uint32_t* run_start,
                        uint32_t nruns, uint32_t ncand, uint32_t rec0, MatchRow* rows, uint32_t* rec_first,
                        unsigned long long* rec_pairs, uint32_t* rank_out, uint32_t* hit_flag, Device& dev, hipStream_t s) {
  if (nruns == 0) return;
  uint32_t shift = 0, m = 0;
  directory_sampling(d.n_hashes, &shift, &m);
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_match_probe, dim3(grid_for(nruns, 256, dev.grid_limit(), dev)), dim3(256), 0, s, d, shift, m, run_hash, run_rec, run_start, nruns,
                     ncand, rec0, rows, rec_first, rec_pairs, rank_out, hit_flag);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("match_probe", s);
}

void launch_match_tally(const MatchDirectory& d, const uint32_t* rank, MatchRow* rows, const uint32_t* rec_first,
                        const unsigned long long* rec_pairs, uint32_t nrec, uint32_t* big_list, uint32_t* big_count, Device& dev,
                        hipStream_t s) {
  if (nrec == 0) return;
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_match_tally, dim3(grid_for(nrec, 4, dev.grid_limit(), dev)), dim3(256), 0, s, d, rank, rows, rec_first, rec_pairs, nrec, big_list,
                     big_count);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("match_tally", s);
}

void launch_match_dense(const MatchDirectory& d, const uint32_t* rank, MatchRow* rows, const uint32_t* rec_first, const uint32_t* big,
                        uint32_t nbig, uint32_t n_nodes, uint32_t* slab, Device& dev, hipStream_t s) {
  if (nbig == 0) return;
  constexpr uint32_t kBlocksPerRecord = 16;
  const uint32_t blocks_per_rec = grid_for(kBlocksPerRecord, 1, kBlocksPerRecord, dev);   // (16 unless the grid cap is lower)
  dev.prof_begin(s);
  HIP_CHECK(hipMemsetAsync(slab, 0, (size_t)nbig * n_nodes * 4, s));
  hipLaunchKernelGGL(k_match_dense_count, dim3(nbig * blocks_per_rec), dim3(256), 0, s, d, rank, rows, rec_first, big, blocks_per_rec,
                     n_nodes, slab);
  hipLaunchKernelGGL(k_match_dense_pick, dim3(nbig), dim3(256), 0, s, slab, n_nodes, big, rows);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("match_tally", s);
}

void launch_match_hit_scatter(const uint64_t* run_hash, const uint32_t* rank, const uint32_t* at, uint32_t nruns, uint64_t* out, Device& dev,
                              hipStream_t s) {
  if (nruns == 0) return;
  hipLaunchKernelGGL(k_match_hit_scatter, dim3(grid_for(nruns, 256, dev.grid_limit(), dev)), dim3(256), 0, s, run_hash, rank, at, nruns, out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace smh
