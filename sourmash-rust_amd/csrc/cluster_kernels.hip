// cluster_kernels.hip -- gfx950 kernels of clustering a resident index (include/sourmash_amd.h, smh_index_cluster; DESIGN.md
// 3.17).  The adjacency is the rule of the thresholded search (search_rule.hpp: survives, through scan_tile) on the counters
// that the index's hash directory fills; the pairs never leave the device.
//
// Components, once per chunk of queries (the chunks are search_self's):
//   k_cl_probe   k_sm_probe's walk, but only c[q][owner] with owner > the query's node is counted: half the atomics.
//   k_cl_link    the grid of k_sm_select; every survivor under kSearchUpperOnly is uf_union(parent, query, node)
//                (union_find.hpp).  Pairs whose roots are equal in a cached view of the forest are filtered with ordinary
//                loads first, as k_uf_runs filters: a stale parent still names a node of the same component.
// and once per call: k_cl_label (label = find), k_cl_best (atomicMax of (score, ~node) per label; roots flagged), a scan of
// the flags, k_cl_gather.
// Greedy: the search kernels' rows are packed into adjacency lists (k_cl_pack), then
//   k_cl_round   one synchronous round: an undecided node that sees a representative among its neighbours of higher priority
//                becomes a member; one that sees neither a representative nor an undecided node there becomes a
//                representative.  Reads only the previous round's states.
//   k_cl_assign  a member's adjacent representatives reduced under the total order (value descending, rank ascending), and
//                atomicMin of the smallest member per representative; k_cl_mark / scan / k_cl_number give the numbers.
// A lane holds a node; adjacency lists longer than kClusterLaneMax are handed round by ballot and walked by the whole wave
// (walk_owners' scheme).  Integer atomics only; no cooperative launch, no workgroup waits for another: a CAS retry in
// uf_union is progress on the lane's own operation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "directory_probe.hpp"
#include "kernels.hpp"
#include "search_rule.hpp"
#include "union_find.hpp"

namespace smh {
namespace {

__global__ __launch_bounds__(256) void k_cl_iota(uint32_t* __restrict__ v, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = i;
}

// shift, m: directory_sampling; q0: the node that the chunk's first query is
__global__ __launch_bounds__(256) void k_cl_probe(MatchDirectory d, uint32_t shift, uint32_t m, const uint64_t* __restrict__ hashes,
                                                  const uint32_t* __restrict__ qoff, uint32_t nq, uint32_t T, uint32_t n, uint32_t q0,
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
    walk_owners(d.owners, hit, b, e, q, t, lane, [&](uint32_t owner, uint32_t qq, uint32_t) {
      if (owner > q0 + qq) atomicAdd(&c[(size_t)qq * n + owner], 1u);
    });
  }
}

// r.self == kSearchUpperOnly
__global__ __launch_bounds__(kTileThreads) void k_cl_link(Rule r, const uint32_t* __restrict__ c, const uint32_t* __restrict__ qoff,
                                                          uint32_t n, uint32_t q0, uint32_t* parent) {
  const uint32_t me = q0 + blockIdx.y;
  if ((blockIdx.x + 1) * kSearchTile <= me + 1) return;   // (uniform) no node of the tile lies above the query
  uint32_t lq, first, common[kSteps], size[kSteps];
  const uint32_t mask = scan_tile(r, c, qoff, n, q0, &lq, &first, common, size);
#pragma unroll
  for (uint32_t s = 0; s < kSteps; s++) {
    if (!((mask >> s) & 1u)) continue;
    uint32_t a = me, b = first + s * 64;
    // ordinary cached loads: equal roots in a stale view prove the two connected (most unions of a dense family end here)
    for (int hop = 0; hop < 64; hop++) { const uint32_t p = parent[a]; if (p == a) break; a = p; }
    for (int hop = 0; hop < 64; hop++) { const uint32_t p = parent[b]; if (p == b) break; b = p; }
    if (a != b) uf_union(parent, a, b);   // (a and b: nodes of the components of the query and of the node)
  }
}

__device__ __forceinline__ uint32_t node_size(const uint64_t* __restrict__ off, uint32_t v) { return (uint32_t)(off[v + 1] - off[v]); }

__global__ __launch_bounds__(256) void k_cl_label(uint32_t* parent, uint32_t* __restrict__ label, unsigned long long* __restrict__ best,
                                                  uint32_t n) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  label[v] = uf_find(parent, v);
  best[v] = 0;
}

// best[l] = the largest (score << 32) | (0xffffffff - v) over the members v of label l: the member first in priority
__global__ __launch_bounds__(256) void k_cl_best(const uint32_t* __restrict__ label, const uint32_t* __restrict__ scores,
                                                 const uint64_t* __restrict__ node_offsets, unsigned long long* best,
                                                 uint32_t* __restrict__ flag, uint32_t n) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const uint32_t l = label[v];
  const uint32_t score = scores ? scores[v] : node_size(node_offsets, v);
  atomicMax(&best[l], ((unsigned long long)score << 32) | (0xffffffffu - v));
  flag[v] = l == v;   // a root is its component's smallest node: the scan of the flags numbers the clusters in that order
}

// flag: scanned (exclusive)
__global__ __launch_bounds__(256) void k_cl_gather(const uint32_t* __restrict__ label, const unsigned long long* __restrict__ best,
                                                   const uint32_t* __restrict__ flag, uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const uint32_t l = label[v];
  out[v] = flag[l];
  out[n + v] = 0xffffffffu - (uint32_t)best[l];
}

__global__ __launch_bounds__(256) void k_cl_pack(const SearchRow* __restrict__ rows, uint32_t R, const uint32_t* __restrict__ query_rows,
                                                 uint32_t nq, uint32_t base, ClusterAdj* __restrict__ adj, uint32_t* __restrict__ start) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < R) adj[base + i] = ClusterAdj{rows[i].node, rows[i].common};
  if (i < nq) start[i] = base + (query_rows ? query_rows[i] : 0u);
}

__global__ __launch_bounds__(256) void k_cl_round(const uint32_t* __restrict__ start, const ClusterAdj* __restrict__ adj,
                                                  const uint32_t* __restrict__ rank, const uint32_t* __restrict__ st_in,
                                                  uint32_t* __restrict__ st_out, uint32_t n, unsigned long long* undecided) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t v0 = blockIdx.x * 256; v0 < n; v0 += gridDim.x * 256) {   // (uniform: whole waves stay for the ballots)
    const uint32_t v = v0 + threadIdx.x;
    const bool ok = v < n;
    uint32_t st = ok ? st_in[v] : (uint32_t)kClusterMember;
    const bool und = ok && st == kClusterUndecided;
    uint32_t b = 0, e = 0, rv = 0;
    if (und) { b = start[v]; e = start[v + 1]; rv = rank[v]; }
    bool any_rep = false, any_und = false;
    const bool longl = und && e - b > kClusterLaneMax;
    if (und && !longl)
      for (uint32_t k = b; k < e; k++) {
        const uint32_t u = adj[k].node;
        if (rank[u] < rv) { const uint32_t su = st_in[u]; any_rep |= su == kClusterRep; any_und |= su == kClusterUndecided; }
      }
    uint64_t lm = __ballot(longl);
    while (lm) {
      const int src = __builtin_ctzll(lm);
      lm &= lm - 1;
      const uint32_t bb = (uint32_t)__shfl((int)b, src), ee = (uint32_t)__shfl((int)e, src), rr = (uint32_t)__shfl((int)rv, src);
      bool r = false, w = false;
      for (uint32_t k = bb + lane; k < ee; k += 64) {
        const uint32_t u = adj[k].node;
        if (rank[u] < rr) { const uint32_t su = st_in[u]; r |= su == kClusterRep; w |= su == kClusterUndecided; }
      }
      const bool R = __ballot(r) != 0, W = __ballot(w) != 0;
      if ((int)lane == src) { any_rep = R; any_und = W; }
    }
    if (und) st = any_rep ? kClusterMember : any_und ? kClusterUndecided : kClusterRep;
    if (ok) st_out[v] = st;
    if (undecided && ok && st == kClusterUndecided) atomicAdd(undecided, 1ull);
  }
}

// the rule's own double of a pair of nodes under a symmetric metric
__device__ __forceinline__ double pair_value(uint32_t metric, uint32_t common, uint32_t la, uint32_t lb) {
  const uint64_t den = metric == kSearchJaccard ? (uint64_t)la + lb - common : (uint64_t)(la < lb ? la : lb);
  return (double)common / (double)den;
}

struct Pick { double value; uint32_t rank, node, common; };
// the total order of a member's choice: value descending, then rank ascending (ranks are distinct)
__device__ __forceinline__ bool better(const Pick& a, const Pick& b) { return a.value > b.value || (a.value == b.value && a.rank < b.rank); }

__device__ __forceinline__ void offer(Pick& best, const ClusterAdj& a, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ st,
                                      uint32_t metric, const uint64_t* __restrict__ node_offsets, uint32_t lv) {
  if (st[a.node] != kClusterRep) return;
  const Pick p{pair_value(metric, a.common, lv, node_size(node_offsets, a.node)), rank[a.node], a.node, a.common};
  if (better(p, best)) best = p;
}

// out: cluster[n] (not written here), representative[n], rep_common[n]; minmem (caller: 0xff bytes) = the smallest member of
// every representative
__global__ __launch_bounds__(256) void k_cl_assign(const uint32_t* __restrict__ start, const ClusterAdj* __restrict__ adj,
                                                   const uint32_t* __restrict__ rank, const uint32_t* __restrict__ st, uint32_t metric,
                                                   const uint64_t* __restrict__ node_offsets, uint32_t n, uint32_t* minmem,
                                                   uint32_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t v0 = blockIdx.x * 256; v0 < n; v0 += gridDim.x * 256) {   // (uniform: whole waves stay for the shuffles)
    const uint32_t v = v0 + threadIdx.x;
    const bool ok = v < n;
    const bool member = ok && st[v] != kClusterRep;
    uint32_t b = 0, e = 0, lv = 0;
    if (ok) lv = node_size(node_offsets, v);
    if (member) { b = start[v]; e = start[v + 1]; }
    Pick best{-1.0, 0xffffffffu, v, lv};   // (a representative keeps this: itself and |S_v|)
    const bool longl = member && e - b > kClusterLaneMax;
    if (member && !longl)
      for (uint32_t k = b; k < e; k++) offer(best, adj[k], rank, st, metric, node_offsets, lv);
    uint64_t lm = __ballot(longl);
    while (lm) {
      const int src = __builtin_ctzll(lm);
      lm &= lm - 1;
      const uint32_t bb = (uint32_t)__shfl((int)b, src), ee = (uint32_t)__shfl((int)e, src), ll = (uint32_t)__shfl((int)lv, src);
      Pick p{-1.0, 0xffffffffu, 0, 0};
      for (uint32_t k = bb + lane; k < ee; k += 64) offer(p, adj[k], rank, st, metric, node_offsets, ll);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {   // better() is a total order on distinct ranks: the lane order cannot matter
        const Pick o{__shfl_xor(p.value, d), (uint32_t)__shfl_xor((int)p.rank, d), (uint32_t)__shfl_xor((int)p.node, d),
                     (uint32_t)__shfl_xor((int)p.common, d)};
        if (better(o, p)) p = o;
      }
      if ((int)lane == src && p.rank != 0xffffffffu) best = p;
    }
    if (ok) {
      out[n + v] = best.node;
      out[2 * (size_t)n + v] = best.common;
      atomicMin(&minmem[best.node], v);
    }
  }
}

// flag (caller: zeroed): 1 at the smallest member of every cluster
__global__ __launch_bounds__(256) void k_cl_mark(const uint32_t* __restrict__ st, const uint32_t* __restrict__ minmem,
                                                 uint32_t* __restrict__ flag, uint32_t n) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v < n && st[v] == kClusterRep) flag[minmem[v]] = 1;
}

// flag: scanned (exclusive)
__global__ __launch_bounds__(256) void k_cl_number(const uint32_t* __restrict__ minmem, const uint32_t* __restrict__ flag,
                                                   uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v < n) out[v] = flag[minmem[out[n + v]]];
}

uint32_t blocks_of(uint32_t n) { return (n + 255) / 256; }

}  // namespace

void cluster_geometry(uint32_t* lane_max, uint32_t* node_tile) {
  if (lane_max) *lane_max = kClusterLaneMax;
  if (node_tile) *node_tile = kSearchTile;
}

void launch_cluster_iota(uint32_t* v, uint32_t n, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_cl_iota, dim3(blocks_of(n)), dim3(256), 0, s, v, n);
  HIP_CHECK(hipGetLastError());
}

void launch_cluster_probe(const MatchDirectory& d, const SearchChunk& ck, Device& dev, hipStream_t s) {
  uint32_t shift = 0, m = 0;
  directory_sampling(d.n_hashes, &shift, &m);
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_cl_probe, dim3(grid_for(ck.T, 256, dev.grid_limit(), dev)), dim3(256), 0, s, d, shift, m, ck.hashes, ck.qoff, ck.nq, ck.T, ck.n, ck.q0,
                     ck.c);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("cluster_probe", s);
}

void launch_cluster_link(const SearchChunk& ck, uint32_t* parent, Device& dev, hipStream_t s) {
  const Rule r{ck.node_offsets, ck.threshold, ck.metric, kSearchUpperOnly, ck.threshold_common};
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_cl_link, dim3(ck.tiles, ck.nq), dim3(kTileThreads), 0, s, r, ck.c, ck.qoff, ck.n, ck.q0, parent);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("cluster_link", s);
}

void launch_cluster_finish_components(uint32_t* parent, const uint32_t* scores, const uint64_t* node_offsets, uint32_t n, uint32_t* work,
                                      uint32_t* out, Device& dev, hipStream_t s) {
  auto* best = reinterpret_cast<unsigned long long*>(work);   // 2 n words, then label[n], flag[n]
  uint32_t* label = work + 2 * (size_t)n;
  uint32_t* flag = label + n;
  const dim3 grid(blocks_of(n));
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_cl_label, grid, dim3(256), 0, s, parent, label, best, n);
  hipLaunchKernelGGL(k_cl_best, grid, dim3(256), 0, s, label, scores, node_offsets, best, flag, n);
  exclusive_scan_u32_dev(flag, n, out + 2 * (size_t)n, dev.scratch, s);
  hipLaunchKernelGGL(k_cl_gather, grid, dim3(256), 0, s, label, best, flag, out, n);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("cluster_finish", s);
}

void launch_cluster_pack(const SearchRow* rows, uint32_t R, const uint32_t* query_rows, uint32_t nq, uint32_t base, ClusterAdj* adj,
                         uint32_t* start, hipStream_t s) {
  hipLaunchKernelGGL(k_cl_pack, dim3(blocks_of(std::max(R, nq))), dim3(256), 0, s, rows, R, query_rows, nq, base, adj, start);
  HIP_CHECK(hipGetLastError());
}

void launch_cluster_round(const uint32_t* start, const ClusterAdj* adj, const uint32_t* rank, const uint32_t* st_in, uint32_t* st_out,
                          uint32_t n, unsigned long long* undecided, Device& dev, hipStream_t s) {
  hipLaunchKernelGGL(k_cl_round, dim3(grid_for(n, 256, dev.grid_limit(), dev)), dim3(256), 0, s, start, adj, rank, st_in, st_out, n, undecided);
  HIP_CHECK(hipGetLastError());
}

void launch_cluster_assign(const uint32_t* start, const ClusterAdj* adj, const uint32_t* rank, const uint32_t* st, uint32_t metric,
                           const uint64_t* node_offsets, uint32_t n, uint32_t* work, uint32_t* out, Device& dev, hipStream_t s) {
  uint32_t* minmem = work;   // n words, then flag[n]
  uint32_t* flag = work + n;
  dev.prof_begin(s);
  HIP_CHECK(hipMemsetAsync(minmem, 0xff, (size_t)n * 4, s));
  hipLaunchKernelGGL(k_cl_assign, dim3(grid_for(n, 256, dev.grid_limit(), dev)), dim3(256), 0, s, start, adj, rank, st, metric, node_offsets, n, minmem, out);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("cluster_assign", s);
  dev.prof_begin(s);
  HIP_CHECK(hipMemsetAsync(flag, 0, (size_t)n * 4, s));
  hipLaunchKernelGGL(k_cl_mark, dim3(blocks_of(n)), dim3(256), 0, s, st, minmem, flag, n);
  exclusive_scan_u32_dev(flag, n, out + 3 * (size_t)n, dev.scratch, s);
  hipLaunchKernelGGL(k_cl_number, dim3(blocks_of(n)), dim3(256), 0, s, minmem, flag, out, n);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("cluster_finish", s);
}

}  // namespace smh
