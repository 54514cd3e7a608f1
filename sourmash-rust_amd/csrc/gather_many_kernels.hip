// gather_many_kernels.hip -- gfx950 kernels of gather for a batch of queries (include/sourmash_amd.h,
// smh_index_gather_many).  Every query is decomposed as gather_kernels.hip decomposes one, but nothing is
// searched or inverted per query: the index's hash directory (MatchDirectory) already holds, per distinct hash, the nodes
// that own it -- the inverted lists of every query at once.  A chunk is a run of consecutive queries whose positions lie
// one after another; position t belongs to query q when qoff[q] <= t < qoff[q + 1].
//
// Once per chunk:
//   k_gm_probe     one lane per position: its rank in U (directory_probe.hpp: the search of k_match_probe) or a miss; on a
//                  hit c0[q][owner] += 1 for every owner.  Owner lists of up to kShortOwners entries are walked by the lane,
//                  longer ones by the whole wave (ballot), as k_gather_subtract walks inverted lists.  The chunk's hits
//                  (position, owner pairs) are summed per wave into one 64-bit atomic.
//   k_gm_size      one workgroup per query: the nodes with c0 >= threshold.  A round's winner has c >= threshold, c <= c0
//                  and wins once, so min(capacity, that number) bounds the query's rows: the host sizes the rows with it.
//   (scan of c0 over the chunk: where the hit list of every (query, node) starts)
//   k_gm_fill      the second pass over the hits: each hit's position into the list of its (query, node) through a cursor.
//                  The cursor is c itself: it counts from 0 up to c0, which is what the rounds start from.
// A round is two launches for the whole chunk and no host work:
//   k_gm_pick      one workgroup per query: arg-max of (c << 32) | ~i over its n counters, the lowest node on ties.  Writes
//                  the row, or sets the query's `done` and takes it off the chunk's `live` count.
//   k_gm_subtract  blockIdx.y is the query.  Walks the winner's hit list, labels the positions nobody consumed, sums their
//                  abundances (one 64-bit atomic per wave) and decrements c[q][owner] for every owner of the position's rank.
// A done query's workgroups return at once.  Integer atomics only; no cooperative launch, no workgroup waits for another.
// query_of, walk_owners and kShortOwners are directory_probe.hpp's (shared with search_many_kernels.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "directory_probe.hpp"
#include "kernels.hpp"
#include "wave_ops.hpp"

namespace smh {
namespace {

constexpr uint32_t kUnassigned = 0xffffffffu;
constexpr uint32_t kPickThreads = 512;

// shift, m: directory_sampling
__global__ __launch_bounds__(256) void k_gm_probe(MatchDirectory d, uint32_t shift, uint32_t m, const uint64_t* __restrict__ hashes,
                                                  const uint32_t* __restrict__ qoff, uint32_t nq, uint32_t T, uint32_t n,
                                                  uint32_t* __restrict__ rank, uint32_t* __restrict__ c0, GatherManyState* st) {
  __shared__ uint64_t samp[kMatchSamples];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  directory_stage_samples(d, shift, m, samp);
  uint64_t wsum = 0;
  for (uint64_t i0 = (uint64_t)blockIdx.x * 256; i0 < T; i0 += (uint64_t)gridDim.x * 256) {
    const uint64_t t64 = i0 + tid;   // (whole waves stay in the loop: walk_owners needs every lane)
    const bool ok = t64 < T;
    const uint32_t t = (uint32_t)t64;
    const uint64_t h = ok ? hashes[t] : 0;
    const uint32_t g = directory_lower_bound(d, samp, shift, m, h, ok);
    const bool hit = ok && g < d.n_hashes && d.U[g] == h;
    uint32_t b = 0, e = 0, q = 0;
    if (hit) { directory_owner_range(d, g, &b, &e); q = query_of(qoff, nq, t); }
    if (ok) rank[t] = hit ? g : kMatchMiss;
    walk_owners(d.owners, hit, b, e, q, t, lane, [&](uint32_t owner, uint32_t qq, uint32_t) { atomicAdd(&c0[(size_t)qq * n + owner], 1u); });
    wsum += e - b;
  }
  wsum = wave_sum_u64(wsum);
  if (lane == 0 && wsum) atomicAdd(&st->hits, (unsigned long long)wsum);
}

__global__ __launch_bounds__(256) void k_gm_size(const uint32_t* __restrict__ c0, uint32_t n, uint32_t threshold, uint32_t* __restrict__ qcnt) {
  __shared__ uint32_t part[4];
  const uint32_t* __restrict__ c = c0 + (size_t)blockIdx.x * n;
  uint32_t k = 0;
  for (uint32_t i = threadIdx.x; i < n; i += 256) k += c[i] >= threshold ? 1u : 0u;
  k = (uint32_t)wave_sum_u64(k);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) qcnt[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void k_gm_fill(MatchDirectory d, const uint32_t* __restrict__ qoff, uint32_t nq, uint32_t T, uint32_t n,
                                                 const uint32_t* __restrict__ rank, const uint32_t* __restrict__ loff,
                                                 uint32_t* __restrict__ cursor, uint32_t* __restrict__ lists) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  for (uint64_t i0 = (uint64_t)blockIdx.x * 256; i0 < T; i0 += (uint64_t)gridDim.x * 256) {
    const uint64_t t64 = i0 + tid;
    const uint32_t t = (uint32_t)t64;
    const uint32_t g = t64 < T ? rank[t] : kMatchMiss;
    const bool hit = g != kMatchMiss;
    uint32_t b = 0, e = 0, q = 0;
    if (hit) { directory_owner_range(d, g, &b, &e); q = query_of(qoff, nq, t); }
    walk_owners(d.owners, hit, b, e, q, t, lane, [&](uint32_t owner, uint32_t qq, uint32_t tt) {
      const size_t at = (size_t)qq * n + owner;
      lists[loff[at] + atomicAdd(&cursor[at], 1u)] = tt;   // (the cursor ends at c0[at] = loff[at + 1] - loff[at])
    });
  }
}

// one workgroup per query; offsets: the nodes' CSR offsets (size_match)
__global__ __launch_bounds__(kPickThreads) void k_gm_pick(const uint32_t* __restrict__ c_all, const uint32_t* __restrict__ c0_all, uint32_t n,
                                                          const uint64_t* __restrict__ offsets, uint32_t threshold,
                                                          const uint64_t* __restrict__ rowoff, GatherRow* __restrict__ rows,
                                                          GatherManyQuery* __restrict__ qs, GatherManyState* st) {
  __shared__ uint64_t part[kPickThreads / 64];
  const uint32_t q = blockIdx.x;
  if (qs[q].done) return;   // (the whole workgroup reads it before thread 0 may write it, behind the barrier)
  const uint32_t* __restrict__ c = c_all + (size_t)q * n;
  uint64_t best = 0;
  for (uint32_t i = threadIdx.x; i < n; i += kPickThreads) {
    const uint64_t key = ((uint64_t)c[i] << 32) | (uint32_t)~i;
    best = key > best ? key : best;
  }
  best = wave_max_u64(best);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (uint32_t k = 1; k < kPickThreads / 64; k++) best = part[k] > best ? part[k] : best;
  const uint32_t cbest = (uint32_t)(best >> 32), i = ~(uint32_t)best, r = qs[q].rounds;
  if (cbest < threshold || r == qs[q].cap) {
    qs[q].done = 1;
    atomicSub(&st->live, 1u);
    return;
  }
  GatherRow row;
  row.match = i; row.common_remaining = cbest; row.common_original = c0_all[(size_t)q * n + i];
  row.size_match = (uint32_t)(offsets[i + 1] - offsets[i]); row.abund_sum = 0;
  rows[rowoff[q] + r] = row;
  qs[q].best = i;
  qs[q].rounds = r + 1;
  atomicMax(&st->max_rounds, r + 1);
}

__global__ __launch_bounds__(256) void k_gm_subtract(MatchDirectory d, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ c0,
                                                     const uint32_t* __restrict__ loff, const uint32_t* __restrict__ lists,
                                                     const uint64_t* __restrict__ counts, uint32_t n, const uint64_t* __restrict__ rowoff,
                                                     uint32_t* __restrict__ c, uint32_t* __restrict__ assigned, GatherRow* __restrict__ rows,
                                                     const GatherManyQuery* __restrict__ qs) {
  const uint32_t q = blockIdx.y;
  if (qs[q].done) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t node = qs[q].best, r = qs[q].rounds - 1;
  const size_t at = (size_t)q * n + node;
  const uint32_t* __restrict__ H = lists + loff[at];
  const uint32_t L = c0[at];
  const uint32_t nw = gridDim.x * 4;
  uint64_t wsum = 0;
  for (uint32_t k0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; k0 < L; k0 += nw * 64) {
    const uint32_t k = k0 + lane;
    bool take = false;
    uint32_t b = 0, e = 0, t = 0;
    if (k < L) {
      t = H[k];
      if (assigned[t] == kUnassigned) {   // a position sits once in a hit list: no other lane looks at this word
        take = true;
        assigned[t] = r;
        wsum += counts ? counts[t] : 1ull;
        directory_owner_range(d, rank[t], &b, &e);
      }
    }
    walk_owners(d.owners, take, b, e, q, t, lane, [&](uint32_t owner, uint32_t qq, uint32_t) { atomicSub(&c[(size_t)qq * n + owner], 1u); });
  }
  wsum = wave_sum_u64(wsum);
  if (lane == 0 && wsum) atomicAdd((unsigned long long*)&rows[rowoff[q] + r].abund_sum, (unsigned long long)wsum);
}

__global__ __launch_bounds__(256) void k_gm_weights(const uint32_t* __restrict__ starts, uint32_t total, uint32_t n, uint64_t* __restrict__ out) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256)
    out[p] = starts ? (uint64_t)((p + 1 < n ? starts[p + 1] : total) - starts[p]) : 1ull;
}


}  // namespace

void launch_gather_many_probe(const MatchDirectory& d, const GatherManyChunk& ck, uint32_t threshold, uint32_t* qcnt, Device& dev,
                              hipStream_t s) {
  uint32_t shift = 0, m = 0;
  directory_sampling(d.n_hashes, &shift, &m);
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_gm_probe, dim3(grid_for(ck.T, 256, dev.grid_limit(), dev)), dim3(256), 0, s, d, shift, m, ck.hashes, ck.qoff, ck.nq, ck.T, ck.n, ck.rank,
                     ck.c0, ck.st);
  hipLaunchKernelGGL(k_gm_size, dim3(ck.nq), dim3(256), 0, s, ck.c0, ck.n, threshold, qcnt);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("gather_many_probe", s);
}

void launch_gather_many_fill(const MatchDirectory& d, const GatherManyChunk& ck, Device& dev, hipStream_t s) {
  const size_t pairs = (size_t)ck.nq * ck.n;
  dev.prof_begin(s);
  HIP_CHECK(hipMemcpyAsync(ck.loff, ck.c0, pairs * 4, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemsetAsync(ck.loff + pairs, 0, 4, s));
  exclusive_scan_u32_dev(ck.loff, pairs + 1, nullptr, dev.scratch, s);
  hipLaunchKernelGGL(k_gm_fill, dim3(grid_for(ck.T, 256, dev.grid_limit(), dev)), dim3(256), 0, s, d, ck.qoff, ck.nq, ck.T, ck.n, ck.rank, ck.loff, ck.c, ck.lists);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("gather_many_fill", s);
}

void launch_gather_many_rounds(const MatchDirectory& d, const GatherManyChunk& ck, const uint64_t* node_offsets, uint32_t threshold,
                               uint32_t sub_grid, uint32_t rounds, Device& dev, hipStream_t s) {
  dev.prof_begin(s);
  for (uint32_t k = 0; k < rounds; k++) {
    hipLaunchKernelGGL(k_gm_pick, dim3(ck.nq), dim3(kPickThreads), 0, s, ck.c, ck.c0, ck.n, node_offsets, threshold, ck.rowoff, ck.rows, ck.qs,
                       ck.st);
    hipLaunchKernelGGL(k_gm_subtract, dim3(sub_grid, ck.nq), dim3(256), 0, s, d, ck.rank, ck.c0, ck.loff, ck.lists, ck.counts, ck.n, ck.rowoff,
                       ck.c, ck.assigned, ck.rows, ck.qs);
  }
  HIP_CHECK(hipGetLastError());
  dev.prof_end("gather_many_rounds", s);
}

void launch_gather_many_weights(const uint32_t* starts, uint32_t total, uint32_t n, uint64_t* out, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_gm_weights, dim3(grid_for(n, 256, 2048, Device::get())), dim3(256), 0, s, starts, total, n, out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace smh
