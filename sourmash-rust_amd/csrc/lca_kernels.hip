// lca_kernels.hip -- gfx950 kernels of the taxonomic LCA on a resident index (include/sourmash_amd.h, "Taxonomic LCA";
// DESIGN.md 3.15).  The taxonomy lives in HBM as one 8-byte entry (parent, depth) per taxon, so a step of the
// depth-equalising walk of lca(a, b) is one load; the node's taxon is one u32 per node.
//
//   k_lca_table          once per index and taxonomy: hash_taxon[g] = the lca over the taxa of the owners of directory rank g.
//                        Owner lists are very uneven: a list of up to kLcaOwnerLaneMax owners is folded by the lane that
//                        holds the rank, a longer one is appended to a compacted list ...
//   k_lca_table_long     ... that gives each of them one wave: a strided read, then a butterfly of lca over the lanes.
//   k_lca_probe          sketch route, one lane per query hash: its rank in the directory (the sampled top in LDS, the last
//                        levels in global memory: directory_probe.hpp), its taxon, the key (query << 32 | taxon) and the flag
//                        of an assigned hash.
//   k_lca_keys           the keys of the assigned hashes compacted (at: the exclusive scan of the flags); the sort and the
//                        run-length pass of sort.hip turn them into the (taxon, count) CSR.
//   k_lca_records        records route, after match's probe: one lane per record folds the join over hash_taxon of the
//                        record's runs when it has at most kLcaRecordLaneMax of them (64 records per wave: reads have 0 to 2);
//                        a longer record is appended to a compacted list ...
//   k_lca_records_long   ... that gives each of them one wave: a strided fold per lane, then a butterfly of the join.
// lca and the join are associative and commutative and every output is an integer: no result depends on which lane folds
// what, on the order of the compacted lists or on the launch geometry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "directory_probe.hpp"
#include "kernels.hpp"

namespace smh {
namespace {

// the deepest common ancestor; kLcaNoTaxon is the identity.  tax[t] = (parent, depth)
__device__ __forceinline__ uint32_t lca2(const uint2* __restrict__ tax, uint32_t a, uint32_t b) {
  if (a == kLcaNoTaxon) return b;
  if (b == kLcaNoTaxon || a == b) return a;
  uint2 ea = tax[a], eb = tax[b];
  while (a != b) {   // (the root, depth 0, is an ancestor of both: the walk ends there at the latest)
    const bool up_a = ea.y >= eb.y, up_b = eb.y >= ea.y;
    if (up_a) { a = ea.x; }
    if (up_b) { b = eb.x; }
    if (a == b) break;
    if (up_a) ea = tax[a];
    if (up_b) eb = tax[b];
  }
  return a;
}

// a summary of a set of taxa: x = where the descent from the root stops, f = it stopped at a branching; x == kLcaNoTaxon:
// the empty set, the identity of the join
struct Summary { uint32_t x, f; };

__device__ __forceinline__ Summary lca_join(const uint2* __restrict__ tax, Summary a, Summary b) {
  if (a.x == kLcaNoTaxon) return b;
  if (b.x == kLcaNoTaxon) return a;
  if (a.x == b.x) return {a.x, a.f | b.f};
  if (tax[a.x].y > tax[b.x].y) { const Summary t = a; a = b; b = t; }   // a is the shallower
  const uint32_t l = lca2(tax, a.x, b.x);
  if (l != a.x) return {l, 1u};
  return a.f ? Summary{a.x, 1u} : b;   // a is a strict ancestor of b
}

__global__ __launch_bounds__(256) void k_lca_table(MatchDirectory d, const uint2* __restrict__ tax, const uint32_t* __restrict__ node_taxon,
                                                   uint32_t* __restrict__ hash_taxon, uint32_t* __restrict__ long_list,
                                                   uint32_t* __restrict__ long_count) {
  for (uint64_t g0 = (uint64_t)blockIdx.x * 256 + threadIdx.x; g0 < d.n_hashes; g0 += (uint64_t)gridDim.x * 256) {
    const uint32_t g = (uint32_t)g0;
    uint32_t b, e;
    directory_owner_range(d, g, &b, &e);
    if (e - b > kLcaOwnerLaneMax) { long_list[atomicAdd(long_count, 1u)] = g; continue; }
    uint32_t t = kLcaNoTaxon;
    for (uint32_t k = b; k < e; k++) t = lca2(tax, t, node_taxon[d.owners[k]]);
    hash_taxon[g] = t;
  }
}

__global__ __launch_bounds__(256) void k_lca_table_long(MatchDirectory d, const uint2* __restrict__ tax,
                                                        const uint32_t* __restrict__ node_taxon, uint32_t* __restrict__ hash_taxon,
                                                        const uint32_t* __restrict__ long_list, const uint32_t* __restrict__ long_count) {
  const uint32_t lane = threadIdx.x & 63, n = *long_count;
  for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {   // (i is the wave's)
    const uint32_t g = long_list[i];
    uint32_t b, e;
    directory_owner_range(d, g, &b, &e);
    uint32_t t = kLcaNoTaxon;
    for (uint32_t k = b + lane; k < e; k += 64) t = lca2(tax, t, node_taxon[d.owners[k]]);
    for (int off = 32; off; off >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)t, off);
      t = lca2(tax, t, o);
    }
    if (lane == 0) hash_taxon[g] = t;
  }
}

// qoff: nq + 1 offsets of the chunk's queries among its T positions
__global__ __launch_bounds__(256) void k_lca_probe(MatchDirectory d, uint32_t shift, uint32_t m, const uint32_t* __restrict__ hash_taxon,
                                                   const uint64_t* __restrict__ hashes, const uint32_t* __restrict__ qoff, uint32_t nq,
                                                   uint32_t T, uint32_t* __restrict__ taxon_out, uint64_t* __restrict__ key_out,
                                                   uint32_t* __restrict__ flag_out) {
  __shared__ uint64_t samp[kMatchSamples];
  directory_stage_samples(d, shift, m, samp);
  const uint32_t nU = d.n_hashes;
  for (uint64_t p0 = (uint64_t)blockIdx.x * 256 + threadIdx.x; p0 < T; p0 += (uint64_t)gridDim.x * 256) {
    const uint32_t p = (uint32_t)p0;
    const uint64_t h = hashes[p];
    const uint32_t g = directory_lower_bound(d, samp, shift, m, h, true);
    uint32_t t = kLcaNoTaxon;
    if (g < nU && d.U[g] == h) t = hash_taxon[g];
    uint32_t lo = 0, hi = nq;   // qoff[lo] <= p < qoff[hi] (empty queries repeat an offset: the last one that starts at or before p)
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (qoff[mid] <= p) lo = mid; else hi = mid;
    }
    taxon_out[p] = t;
    key_out[p] = ((uint64_t)lo << 32) | t;
    flag_out[p] = t != kLcaNoTaxon ? 1u : 0u;
  }
}

__global__ __launch_bounds__(256) void k_lca_keys(const uint64_t* __restrict__ key, const uint32_t* __restrict__ at, uint32_t T,
                                                  uint64_t* __restrict__ out) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < T; p += (uint64_t)gridDim.x * 256) {
    const uint64_t k = key[p];
    if ((uint32_t)k != kLcaNoTaxon) out[at[p]] = k;
  }
}

// the fold of runs [first + k0, first + cnt) of a record in steps of `step`, and how many of them were assigned
__device__ __forceinline__ Summary fold_runs(const uint2* __restrict__ tax, const uint32_t* __restrict__ hash_taxon,
                                             const uint32_t* __restrict__ rank, uint32_t first, uint32_t k0, uint32_t cnt, uint32_t step,
                                             uint32_t* assigned) {
  Summary s{kLcaNoTaxon, 0u};
  uint32_t a = 0;
  for (uint32_t k = k0; k < cnt; k += step) {
    const uint32_t g = rank[first + k];
    if (g == kMatchMiss) continue;
    const uint32_t t = hash_taxon[g];
    if (t == kLcaNoTaxon) continue;
    a++;
    s = lca_join(tax, s, Summary{t, 0u});
  }
  *assigned = a;
  return s;
}

__device__ __forceinline__ void write_lca_row(LcaRow* __restrict__ out, const MatchRow& m, uint32_t assigned, Summary s) {
  LcaRow r;
  r.windows = m.windows; r.distinct = m.distinct; r.hit_distinct = m.hit_distinct; r.assigned_distinct = assigned;
  r.taxon = s.x;
  r.status = s.x == kLcaNoTaxon ? 0u : s.f ? 2u : 1u;
  *out = r;
}

// rows, rec_first, rank: of the fold's nrec records, as k_match_probe left them
__global__ __launch_bounds__(256) void k_lca_records(const uint2* __restrict__ tax, const uint32_t* __restrict__ hash_taxon,
                                                     const uint32_t* __restrict__ rank, const MatchRow* __restrict__ rows,
                                                     const uint32_t* __restrict__ rec_first, uint32_t nrec, LcaRow* __restrict__ out,
                                                     uint32_t* __restrict__ big_list, uint32_t* __restrict__ big_count) {
  for (uint64_t r0 = (uint64_t)blockIdx.x * 256 + threadIdx.x; r0 < nrec; r0 += (uint64_t)gridDim.x * 256) {
    const uint32_t r = (uint32_t)r0;
    const MatchRow m = rows[r];
    if (m.hit_distinct == 0) { write_lca_row(out + r, m, 0, Summary{kLcaNoTaxon, 0u}); continue; }
    if (m.distinct > kLcaRecordLaneMax) { big_list[atomicAdd(big_count, 1u)] = r; continue; }
    uint32_t a;
    const Summary s = fold_runs(tax, hash_taxon, rank, rec_first[r], 0, m.distinct, 1, &a);
    write_lca_row(out + r, m, a, s);
  }
}

__global__ __launch_bounds__(256) void k_lca_records_long(const uint2* __restrict__ tax, const uint32_t* __restrict__ hash_taxon,
                                                          const uint32_t* __restrict__ rank, const MatchRow* __restrict__ rows,
                                                          const uint32_t* __restrict__ rec_first, LcaRow* __restrict__ out,
                                                          const uint32_t* __restrict__ big_list, const uint32_t* __restrict__ big_count) {
  const uint32_t lane = threadIdx.x & 63, n = *big_count;
  for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {   // (i is the wave's)
    const uint32_t r = big_list[i];
    const MatchRow m = rows[r];
    uint32_t a;
    Summary s = fold_runs(tax, hash_taxon, rank, rec_first[r], lane, m.distinct, 64, &a);
    for (int off = 32; off; off >>= 1) {
      const Summary o{(uint32_t)__shfl_xor((int)s.x, off), (uint32_t)__shfl_xor((int)s.f, off)};
      a += (uint32_t)__shfl_xor((int)a, off);
      s = lca_join(tax, s, o);
    }
    if (lane == 0) write_lca_row(out + r, m, a, s);
  }
}


}  // namespace

void lca_geometry(uint32_t* owner_lane_max, uint32_t* record_lane_max, uint32_t* threads) {
  if (owner_lane_max) *owner_lane_max = kLcaOwnerLaneMax;
  if (record_lane_max) *record_lane_max = kLcaRecordLaneMax;
  if (threads) *threads = kLcaThreads;
}

void launch_lca_table(const MatchDirectory& d, const LcaTaxonomy& t, uint32_t* hash_taxon, uint32_t* long_list, uint32_t* long_count,
                      Device& dev, hipStream_t s) {
  if (d.n_hashes == 0) return;
  const uint2* tax = reinterpret_cast<const uint2*>(t.tax);
  dev.prof_begin(s);
  HIP_CHECK(hipMemsetAsync(long_count, 0, 4, s));
  hipLaunchKernelGGL(k_lca_table, dim3(grid_for(d.n_hashes, 256, dev.grid_limit(), dev)), dim3(256), 0, s, d, tax, t.node_taxon, hash_taxon, long_list,
                     long_count);
  // (the long lists number at most n_pairs / (kLcaOwnerLaneMax + 1): the grid is sized for that, the kernel reads the count)
  hipLaunchKernelGGL(k_lca_table_long, dim3(grid_for(d.n_pairs / (kLcaOwnerLaneMax + 1) + 1, 4, dev.grid_limit(), dev)), dim3(256), 0, s, d, tax,
                     t.node_taxon, hash_taxon, long_list, long_count);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("lca_table", s);
}

void launch_lca_probe(const MatchDirectory& d, const uint32_t* hash_taxon, const uint64_t* hashes, const uint32_t* qoff, uint32_t nq,
                      uint32_t T, uint32_t* taxon_out, uint64_t* key_out, uint32_t* flag_out, Device& dev, hipStream_t s) {
  if (T == 0) return;
  uint32_t shift = 0, m = 0;
  directory_sampling(d.n_hashes, &shift, &m);
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_lca_probe, dim3(grid_for(T, 256, dev.grid_limit(), dev)), dim3(256), 0, s, d, shift, m, hash_taxon, hashes, qoff, nq, T, taxon_out,
                     key_out, flag_out);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("lca_probe", s);
}

void launch_lca_keys(const uint64_t* key, const uint32_t* at, uint32_t T, uint64_t* out, Device& dev, hipStream_t s) {
  if (T == 0) return;
  hipLaunchKernelGGL(k_lca_keys, dim3(grid_for(T, 256, dev.grid_limit(), dev)), dim3(256), 0, s, key, at, T, out);
  HIP_CHECK(hipGetLastError());
}

void launch_lca_records(const LcaTaxonomy& t, const uint32_t* hash_taxon, const uint32_t* rank, const MatchRow* rows,
                        const uint32_t* rec_first, uint32_t nrec, LcaRow* out, uint32_t* big_list, uint32_t* big_count, Device& dev,
                        hipStream_t s) {
  if (nrec == 0) return;
  const uint2* tax = reinterpret_cast<const uint2*>(t.tax);
  dev.prof_begin(s);
  HIP_CHECK(hipMemsetAsync(big_count, 0, 4, s));
  hipLaunchKernelGGL(k_lca_records, dim3(grid_for(nrec, 256, dev.grid_limit(), dev)), dim3(256), 0, s, tax, hash_taxon, rank, rows, rec_first, nrec, out,
                     big_list, big_count);
  hipLaunchKernelGGL(k_lca_records_long, dim3(grid_for(nrec, 4, dev.grid_limit(), dev)), dim3(256), 0, s, tax, hash_taxon, rank, rows, rec_first, out,
                     big_list, big_count);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("lca_records", s);
}

}  // namespace smh
