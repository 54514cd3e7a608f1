// nearest_kernels.hip -- gfx950 kernels of the nearest neighbours of a batch of queries (include/sourmash_amd.h,
// smh_index_nearest_many): of the rows the thresholded search reports for a query, the best k by (value
// descending, node ascending).  A chunk's front half is search_many's (the probe and the select of
// search_many_kernels.hip): c[q][i] = |Q_q ^ S_i| and tile_rows, scanned, the survivors of the rule per (query, tile).
//
// Once per chunk, behind them:
//   k_nn_clamp  a tile keeps min(survivors, k) candidates, a query min(its survivors, k) rows.
//   (ONE scan over both, the rows' counts behind the candidates': where each tile's candidates start, and -- counted from
//   row_at[0], the chunk's candidates -- where each query's rows start; the two totals are what the host reads)
//   k_nn_tile   blockIdx.y is the query, blockIdx.x a tile of kSearchTile nodes: the survivors' keys (value bits, node) go
//               into LDS, packed; the workgroup sorts them there and the tile's first min(survivors, k) go to its place in
//               the candidate buffer.
//   k_nn_merge  one workgroup per query: its tiles' candidates lie one after another; they are folded into the running best
//               k in LDS, kNearestSlots - k per step, each step one sort.  Then the rows are written at the query's offset:
//               common and the node's size are read again for the k kept nodes only.
// The key orders itself: the value is a positive double, so its bit pattern compared as an unsigned integer is its order,
// and a node appears once per query, so no two keys of a query are equal -- the sorted order does not depend on the
// network, the grid or the chunk.  An empty slot holds (0, ~0): behind every key.
// The sort is a bitonic network over the smallest power of two that holds the keys, every stage through LDS with a barrier
// behind it (hashes and nodes in arrays of their own: 8- and 4-byte strides, no 12-byte records across the banks).  No
// atomics, no cooperative launch, no workgroup waits for another; every barrier is reached by the whole workgroup: what
// decides a return or a trip count is read from global memory by every thread alike.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "search_rule.hpp"

namespace smh {
namespace {

static_assert(kNearestSlots >= kSearchTile && (kNearestSlots & (kNearestSlots - 1)) == 0, "a tile's survivors fit the slots");
static_assert(kNearestMaxK < kNearestSlots, "a merge step takes at least one candidate");

constexpr uint32_t kEmptyNode = 0xffffffffu;

__device__ __forceinline__ bool key_before(uint64_t va, uint32_t na, uint64_t vb, uint32_t nb) {
  return va > vb || (va == vb && na < nb);
}

__device__ __forceinline__ uint32_t pow2_at_least(uint32_t x) {   // x >= 1
  return x <= 1 ? 1u : 1u << (32 - __clz(x - 1));
}

// slots [0, P) of v / nd in key order (P a power of two up to kNearestSlots, the same for every thread).  The caller has
// put a barrier behind its writes; the last stage is followed by one.
__device__ __forceinline__ void sort_slots(uint64_t* v, uint32_t* nd, uint32_t P) {
  for (uint32_t k = 2; k <= P; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < P / 2; t += kTileThreads) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // the pair's lower slot: bit j clear
        const uint32_t l = i | j;
        const uint64_t va = v[i], vb = v[l];
        const uint32_t na = nd[i], nb = nd[l];
        const bool swap = (i & k) == 0 ? key_before(vb, nb, va, na) : key_before(va, na, vb, nb);
        if (swap) { v[i] = vb; v[l] = va; nd[i] = nb; nd[l] = na; }
      }
      __syncthreads();
    }
  }
}

// slots [from, P) made empty
__device__ __forceinline__ void pad_slots(uint64_t* v, uint32_t* nd, uint32_t from, uint32_t P) {
  for (uint32_t t = from + threadIdx.x; t < P; t += kTileThreads) { v[t] = 0; nd[t] = kEmptyNode; }
}

// tile_rows: scanned (exclusive; cells + 1 entries).  cand_at: cells + 1, row_at = cand_at + cells + 1: nq + 1 (the last of
// each: 0, so that the scan over all of them leaves the candidates' total in cand_at[cells] and in row_at[0]).
__global__ __launch_bounds__(256) void k_nn_clamp(const uint32_t* __restrict__ tile_rows, uint32_t cells, uint32_t tiles, uint32_t nq,
                                                  uint32_t k, uint32_t* __restrict__ cand_at, uint32_t* __restrict__ row_at) {
  const uint64_t items = (uint64_t)cells + 1 + nq + 1;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (uint64_t)gridDim.x * 256) {
    if (i < cells) {
      cand_at[i] = min(tile_rows[i + 1] - tile_rows[i], k);
    } else if (i == cells) {
      cand_at[cells] = 0;
    } else {
      const uint32_t q = (uint32_t)(i - cells - 1);
      row_at[q] = q < nq ? min(tile_rows[(size_t)(q + 1) * tiles] - tile_rows[(size_t)q * tiles], k) : 0;
    }
  }
}

// tile_rows, cand_at: scanned
__global__ __launch_bounds__(kTileThreads) void k_nn_tile(Rule r, const uint32_t* __restrict__ c, const uint32_t* __restrict__ qoff,
                                                          uint32_t n, uint32_t q0, uint32_t tiles, const uint32_t* __restrict__ tile_rows,
                                                          const uint32_t* __restrict__ cand_at, uint64_t* __restrict__ cand_v,
                                                          uint32_t* __restrict__ cand_n) {
  __shared__ uint64_t s_v[kSearchTile];
  __shared__ uint32_t s_n[kSearchTile];
  __shared__ uint32_t part[kTileThreads / 64];
  const size_t cell = (size_t)blockIdx.y * tiles + blockIdx.x;
  const uint32_t S = tile_rows[cell + 1] - tile_rows[cell];
  if (S == 0) return;   // (uniform)
  const uint32_t start = cand_at[cell], keep = cand_at[cell + 1] - start;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t lq, first, common[kSteps], size[kSteps];
  const uint32_t mask = scan_tile(r, c, qoff, n, q0, &lq, &first, common, size);
  uint64_t votes[kSteps];
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t s = 0; s < kSteps; s++) { votes[s] = __ballot((mask >> s) & 1u); cnt += (uint32_t)__popcll(votes[s]); }
  if (lane == 0) part[wave] = cnt;
  __syncthreads();
  uint32_t at = 0;
  for (uint32_t w = 0; w < wave; w++) at += part[w];
  const uint64_t below = (1ull << lane) - 1;
#pragma unroll
  for (uint32_t s = 0; s < kSteps; s++) {
    if ((mask >> s) & 1u) {
      const uint32_t pos = at + (uint32_t)__popcll(votes[s] & below);   // (< S: the select counted the same survivors)
      if (pos < kSearchTile) {
        s_v[pos] = (uint64_t)__double_as_longlong(metric_value(r, common[s], lq, size[s]));
        s_n[pos] = first + s * 64;
      }
    }
    at += (uint32_t)__popcll(votes[s]);
  }
  const uint32_t P = pow2_at_least(S);
  pad_slots(s_v, s_n, S, P);
  __syncthreads();
  sort_slots(s_v, s_n, P);
  for (uint32_t t = threadIdx.x; t < keep; t += kTileThreads) { cand_v[start + t] = s_v[t]; cand_n[start + t] = s_n[t]; }
}

// cand_at, row_at: scanned as one array (row_at[0] = the chunk's candidates: the rows count from there).  k <= kNearestMaxK.
__global__ __launch_bounds__(kTileThreads) void k_nn_merge(const uint32_t* __restrict__ c, const uint32_t* __restrict__ qoff,
                                                           const uint64_t* __restrict__ node_offsets, uint32_t n, uint32_t tiles, uint32_t k,
                                                           const uint32_t* __restrict__ cand_at, const uint64_t* __restrict__ cand_v,
                                                           const uint32_t* __restrict__ cand_n, const uint32_t* __restrict__ row_at,
                                                           SearchRow* __restrict__ rows) {
  __shared__ uint64_t s_v[kNearestSlots];
  __shared__ uint32_t s_n[kNearestSlots];
  const uint32_t q = blockIdx.x;
  const uint32_t out = row_at[q] - row_at[0], kq = row_at[q + 1] - row_at[q];
  if (kq == 0) return;   // (uniform)
  const uint32_t a = cand_at[(size_t)q * tiles], m = cand_at[(size_t)(q + 1) * tiles] - a;
  uint32_t held = 0;
  for (uint32_t pos = 0; pos < m;) {
    const uint32_t take = min(m - pos, kNearestSlots - k);
    for (uint32_t t = threadIdx.x; t < take; t += kTileThreads) { s_v[held + t] = cand_v[a + pos + t]; s_n[held + t] = cand_n[a + pos + t]; }
    const uint32_t total = held + take, P = pow2_at_least(total);   // (<= kNearestSlots: held <= k)
    pad_slots(s_v, s_n, total, P);
    __syncthreads();
    sort_slots(s_v, s_n, P);
    held = min(total, k);
    pos += take;
  }
  // (kq <= held: a query whose tiles were all kept whole holds every survivor, any other holds k)
  const uint32_t lq = qoff[q + 1] - qoff[q];
  for (uint32_t t = threadIdx.x; t < kq; t += kTileThreads) {
    const uint32_t i = s_n[t];
    if (i < n)   // (always: kq <= held keys, none of them an empty slot)
      rows[out + t] = SearchRow{i, c[(size_t)q * n + i], (uint32_t)(node_offsets[i + 1] - node_offsets[i]), lq};
  }
}

}  // namespace

void nearest_geometry(uint32_t* max_k, uint32_t* node_tile, uint32_t* merge_slots) {
  if (max_k) *max_k = kNearestMaxK;
  if (node_tile) *node_tile = kSearchTile;
  if (merge_slots) *merge_slots = kNearestSlots;
}

void launch_nearest_clamp(const SearchChunk& ck, const NearestChunk& nc, Device& dev, hipStream_t s) {
  const uint32_t cells = ck.nq * ck.tiles;
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_nn_clamp, dim3(grid_for((uint64_t)cells + ck.nq + 2, 256, dev.grid_limit(), dev)), dim3(256), 0, s, ck.tile_rows, cells,
                     ck.tiles, ck.nq, nc.k, nc.cand_at, nc.row_at);
  HIP_CHECK(hipGetLastError());
  exclusive_scan_u32_dev(nc.cand_at, (size_t)cells + ck.nq + 2, nullptr, dev.scratch, s);   // (row_at lies behind cand_at)
  dev.prof_end("nearest_clamp", s);
}

void launch_nearest_tile(const SearchChunk& ck, const NearestChunk& nc, Device& dev, hipStream_t s) {
  const Rule r{ck.node_offsets, ck.threshold, ck.metric, ck.self, ck.threshold_common};
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_nn_tile, dim3(ck.tiles, ck.nq), dim3(kTileThreads), 0, s, r, ck.c, ck.qoff, ck.n, ck.q0, ck.tiles, ck.tile_rows,
                     nc.cand_at, nc.cand_v, nc.cand_n);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("nearest_tile", s);
}

void launch_nearest_merge(const SearchChunk& ck, const NearestChunk& nc, SearchRow* rows, Device& dev, hipStream_t s) {
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_nn_merge, dim3(ck.nq), dim3(kTileThreads), 0, s, ck.c, ck.qoff, ck.node_offsets, ck.n, ck.tiles, nc.k, nc.cand_at,
                     nc.cand_v, nc.cand_n, nc.row_at, rows);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("nearest_merge", s);
}

}  // namespace smh
