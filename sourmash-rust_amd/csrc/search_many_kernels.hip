// search_many_kernels.hip -- gfx950 kernels of the thresholded search of a batch of queries (include/sourmash_amd.h,
// smh_index_search_many).  The index's hash directory (MatchDirectory) holds, per distinct hash, the nodes
// that own it, so |Q_q ^ S_i| of every (query, node) pair of a chunk is one counter that the probe of the chunk's positions
// fills; nothing walks the resident hashes.  A chunk is a run of consecutive queries whose positions lie one after another;
// position t belongs to query q when qoff[q] <= t < qoff[q + 1].
//
// Once per chunk:
//   k_sm_probe   one lane per position: its rank in U (directory_probe.hpp: the search of k_match_probe) or a miss; on a hit
//                c[q][owner] += 1 for every owner, the lists walked as k_gm_probe walks them (walk_owners).
//   k_sm_select  blockIdx.y is the query, blockIdx.x a tile of kSearchTile nodes: the rule on every counter of the tile, the
//                survivors counted into tile_rows[q][tile].
//   (scan of tile_rows: where each tile's rows start; the last entry is the chunk's rows, which the host reads to size them)
//   k_sm_emit    the same pass again: a survivor's place is its tile's start + the survivors in front of it inside the tile
//                (ballot / popcount inside a wave, the waves of a workgroup in order), so rows ascend by node with no cursor.
// A thread of select / emit holds 4 nodes: wave w of the workgroup takes nodes [256 w, 256 w + 256) of the tile in 4 steps
// of 64.  Integer atomics only, in the probe; no cooperative launch, no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "directory_probe.hpp"
#include "kernels.hpp"
#include "search_rule.hpp"

namespace smh {
namespace {

// shift, m: directory_sampling
__global__ __launch_bounds__(256) void k_sm_probe(MatchDirectory d, uint32_t shift, uint32_t m, const uint64_t* __restrict__ hashes,
                                                  const uint32_t* __restrict__ qoff, uint32_t nq, uint32_t T, uint32_t n,
                                                  uint32_t* __restrict__ c) {
  __shared__ uint64_t samp[kMatchSamples];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  directory_stage_samples(d, shift, m, samp);
  for (uint64_t i0 = (uint64_t)blockIdx.x * 256; i0 < T; i0 += (uint64_t)gridDim.x * 256) {
    const uint64_t t64 = i0 + tid;   // (whole waves stay in the loop: walk_owners needs every lane)
    const bool ok = t64 < T;
    const uint32_t t = (uint32_t)t64;
    const uint64_t h = ok ? hashes[t] : 0;
    const uint32_t g = directory_lower_bound(d, samp, shift, m, h, ok);
    const bool hit = ok && g < d.n_hashes && d.U[g] == h;
    uint32_t b = 0, e = 0, q = 0;
    if (hit) { directory_owner_range(d, g, &b, &e); q = query_of(qoff, nq, t); }
    walk_owners(d.owners, hit, b, e, q, t, lane, [&](uint32_t owner, uint32_t qq, uint32_t) { atomicAdd(&c[(size_t)qq * n + owner], 1u); });
  }
}

__global__ __launch_bounds__(kTileThreads) void k_sm_select(Rule r, const uint32_t* __restrict__ c, const uint32_t* __restrict__ qoff,
                                                            uint32_t n, uint32_t q0, uint32_t tiles, uint32_t* __restrict__ tile_rows) {
  __shared__ uint32_t part[kTileThreads / 64];
  uint32_t lq, first, common[kSteps], size[kSteps];
  const uint32_t mask = scan_tile(r, c, qoff, n, q0, &lq, &first, common, size);
  uint32_t k = 0;
#pragma unroll
  for (uint32_t s = 0; s < kSteps; s++) k += (uint32_t)__popcll(__ballot((mask >> s) & 1u));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
    for (uint32_t w = 0; w < kTileThreads / 64; w++) sum += part[w];
    tile_rows[(size_t)blockIdx.y * tiles + blockIdx.x] = sum;
  }
}

// tile_rows: scanned (exclusive)
__global__ __launch_bounds__(kTileThreads) void k_sm_emit(Rule r, const uint32_t* __restrict__ c, const uint32_t* __restrict__ qoff,
                                                          uint32_t n, uint32_t q0, uint32_t tiles, const uint32_t* __restrict__ tile_rows,
                                                          SearchRow* __restrict__ rows, uint32_t* __restrict__ query_rows) {
  __shared__ uint32_t part[kTileThreads / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t start = tile_rows[(size_t)blockIdx.y * tiles + blockIdx.x];
  if (blockIdx.x == 0 && threadIdx.x == 0) query_rows[blockIdx.y] = start;
  if (tile_rows[(size_t)blockIdx.y * tiles + blockIdx.x + 1] == start) return;   // (uniform; the array ends with the total)
  uint32_t lq, first, common[kSteps], size[kSteps];
  const uint32_t mask = scan_tile(r, c, qoff, n, q0, &lq, &first, common, size);
  uint64_t votes[kSteps];
  uint32_t k = 0;
#pragma unroll
  for (uint32_t s = 0; s < kSteps; s++) { votes[s] = __ballot((mask >> s) & 1u); k += (uint32_t)__popcll(votes[s]); }
  if (lane == 0) part[wave] = k;
  __syncthreads();
  uint32_t at = start;
  for (uint32_t w = 0; w < wave; w++) at += part[w];
  const uint64_t below = (1ull << lane) - 1;
#pragma unroll
  for (uint32_t s = 0; s < kSteps; s++) {
    if ((mask >> s) & 1u) rows[at + (uint32_t)__popcll(votes[s] & below)] = SearchRow{first + s * 64, common[s], size[s], lq};
    at += (uint32_t)__popcll(votes[s]);
  }
}


Rule rule_of(const SearchChunk& ck) { return {ck.node_offsets, ck.threshold, ck.metric, ck.self, ck.threshold_common}; }

}  // namespace

void search_geometry(uint32_t* short_owners, uint32_t* node_tile, uint32_t* max_queries) {
  if (short_owners) *short_owners = kShortOwners;
  if (node_tile) *node_tile = kSearchTile;
  if (max_queries) *max_queries = kSearchMaxQueries;
}

void launch_search_many_probe(const MatchDirectory& d, const SearchChunk& ck, Device& dev, hipStream_t s) {
  uint32_t shift = 0, m = 0;
  directory_sampling(d.n_hashes, &shift, &m);
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_sm_probe, dim3(grid_for(ck.T, 256, dev.grid_limit(), dev)), dim3(256), 0, s, d, shift, m, ck.hashes, ck.qoff, ck.nq, ck.T, ck.n, ck.c);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("search_many_probe", s);
}

void launch_search_many_select(const SearchChunk& ck, Device& dev, hipStream_t s) {
  const size_t cells = (size_t)ck.nq * ck.tiles;
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_sm_select, dim3(ck.tiles, ck.nq), dim3(kTileThreads), 0, s, rule_of(ck), ck.c, ck.qoff, ck.n, ck.q0, ck.tiles,
                     ck.tile_rows);
  HIP_CHECK(hipMemsetAsync(ck.tile_rows + cells, 0, 4, s));
  exclusive_scan_u32_dev(ck.tile_rows, cells + 1, nullptr, dev.scratch, s);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("search_many_select", s);
}

void launch_search_many_emit(const SearchChunk& ck, SearchRow* rows, uint32_t* query_rows, Device& dev, hipStream_t s) {
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_sm_emit, dim3(ck.tiles, ck.nq), dim3(kTileThreads), 0, s, rule_of(ck), ck.c, ck.qoff, ck.n, ck.q0, ck.tiles, ck.tile_rows,
                     rows, query_rows);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("search_many_emit", s);
}

}  // namespace smh
