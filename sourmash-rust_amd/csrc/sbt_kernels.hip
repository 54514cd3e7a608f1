// sbt_kernels.hip -- gfx950 kernels of the Nodegraph's batched forms and of the resident Sequence Bloom Tree
// (reference src/index/nodegraph.rs, src/index/sbt.rs:147-175, 207-277).
//
//   k_sbt_bins      hash % tablesize for every (query hash, table), once per batch: every node of a tree has the same
//                   table sizes, so a hash's bins are the same at every node.  gfx950 has no integer divide; the modulo
//                   is a 64-bit multiply-high by floor((2^64 - 1) / size) and one correction (fastmod below).
//   k_sbt_nodes     one level of the level-synchronous walk: one workgroup per node, the node's tables staged in LDS
//                   once when they fit (W * 8 <= 64 KiB; the sourmash default of 4 x 1e5 bits is 50 KB), else read from
//                   global memory; one wavefront per waiting query counts the query hashes whose bit is set in every
//                   table.  Passing pairs count their internal children for the next level and append their leaf
//                   children to the (leaf, query) list.
//   k_sbt_fill      scatters the passing pairs' queries into the next level's per-node lists (after a scan of the counts).
//   k_sbt_leaves    the (leaf, query) list: one wavefront per pair through the compare kernels' union walk
//                   (compare_pair.hpp), passing pairs appended to the hit list.
//   k_sbt_count_leaves / k_sbt_or_level / k_sbt_popcount   the tree build: leaf hashes OR-ed into their parents with
//                   64-bit atomics, then one plain OR pass per level bottom-up, then popcount of table 0 per node.
//   k_ng_*          Nodegraph::count / get over a batch (count in array order: a per-table min-index pass decides which
//                   hash sets a bin first).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compare_pair.hpp"
#include "sbt.hpp"
#include "wave_ops.hpp"

namespace smh {
namespace {

// h % s for any u64 h and 1 <= s < 2^32, with m = floor((2^64 - 1) / s).  m >= 2^64 / s - 1, so
// q = mulhi(h, m) > h / s - 2 and q <= h * m / 2^64 < h / s: q is floor(h / s) or one less, and r = h - q s < 2 s.
__device__ __forceinline__ uint32_t fastmod(uint64_t h, uint64_t m, uint32_t s) {
  const uint64_t q = __umul64hi(h, m);
  uint64_t r = h - q * (uint64_t)s;
  if (r >= s) r -= s;
  return (uint32_t)r;
}

__global__ __launch_bounds__(256) void k_sbt_bins(const uint64_t* __restrict__ hashes, uint64_t n,
                                                  const uint32_t* __restrict__ sizes, const uint64_t* __restrict__ magic,
                                                  uint32_t T, uint32_t* __restrict__ bins) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t h = hashes[i];
    for (uint32_t t = 0; t < T; t++) bins[i * T + t] = fastmod(h, magic[t], sizes[t]);
  }
}

template <bool InLds>
__global__ __launch_bounds__(256) void k_sbt_nodes(SbtDev t, SbtQueries qs, SbtLevel lv, double threshold, uint32_t containment) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds_tab[];
  const uint32_t g = blockIdx.x;
  const uint32_t cnt = lv.cnt[g];
  if (cnt == 0) return;
  const uint32_t node = lv.n0 + g;
  const uint64_t* tab = t.tables + (uint64_t)node * t.W;
  if (InLds) {
    for (uint32_t w = threadIdx.x; w < t.W; w += blockDim.x) lds_tab[w] = tab[w];
    __syncthreads();
    tab = lds_tab;
  }
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const uint32_t base = lv.off[g];
  const uint64_t mnb = t.min_n_below[node];
  for (uint32_t k = wave; k < cnt; k += nwaves) {
    const uint32_t q = lv.q[base + k];
    const uint64_t qo = qs.off[q], qe = qs.off[q + 1];
    uint64_t matches = 0;
    for (uint64_t i = qo + lane; i < qe; i += 64) {
      const uint32_t* b = qs.bins + i * t.T;
      bool all = true;
      for (uint32_t tt = 0; tt < t.T && all; tt++) {
        const uint32_t bin = b[tt];
        all = (tab[t.woff[tt] + (bin >> 6)] >> (bin & 63)) & 1;
      }
      matches += all;
    }
    matches = wave_sum_u64(matches);
    if (lane == 0) {
      const uint64_t nq = qe - qo;
      double value = 0.0;   // an empty query: 0.0 (sbt.rs:224-226, 252-254)
      bool err = false;
      if (nq != 0) {
        if (containment) value = (double)matches / (double)nq;
        else if (mnb == kNoMinNBelow) err = true;
        else value = (double)matches / (double)mnb;
      }
      bool pass = !err && value > threshold;
      if (err) atomicMin(lv.err_q, q);
      lv.pass[base + k] = pass ? 1 : 0;
      if (pass) {
        for (uint32_t c = 0; c < t.d; c++) {
          const uint32_t ch = t.child[(uint64_t)node * t.d + c];
          if (ch == kChildNone) continue;
          if (ch & kChildLeaf) {
            const unsigned int at = atomicAdd(lv.lp_n, 1u);
            if (at < lv.lp_cap) lv.lp[at] = make_uint2(ch & ~kChildLeaf, q);
          } else {
            atomicAdd(&lv.next_cnt[ch - lv.next_n0], 1u);
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_sbt_fill(SbtDev t, SbtLevel lv) {
  const uint32_t g = blockIdx.x;
  const uint32_t cnt = lv.cnt[g];
  const uint32_t node = lv.n0 + g;
  const uint32_t base = lv.off[g];
  for (uint32_t k = threadIdx.x; k < cnt; k += blockDim.x) {
    if (!lv.pass[base + k]) continue;
    const uint32_t q = lv.q[base + k];
    for (uint32_t c = 0; c < t.d; c++) {
      const uint32_t ch = t.child[(uint64_t)node * t.d + c];
      if (ch == kChildNone || (ch & kChildLeaf)) continue;
      const uint32_t j = ch - lv.next_n0;
      lv.next_q[lv.next_off[j] + atomicAdd(&lv.next_fill[j], 1u)] = q;
    }
  }
}

template <bool InLds>
__global__ __launch_bounds__(64) void k_sbt_leaves(SbtDev t, SbtQueries qs, const uint2* __restrict__ lp,
                                                   const unsigned int* __restrict__ lp_n, uint32_t cap, double threshold,
                                                   uint32_t containment, unsigned long long* __restrict__ hits,
                                                   unsigned int* __restrict__ hits_n) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds64[];
  const int lane = threadIdx.x;
  const uint32_t npairs = min((uint32_t)*lp_n, cap);
  for (uint32_t pid = blockIdx.x; pid < npairs; pid += gridDim.x) {
    const uint2 pr = lp[pid];
    const uint64_t ao = t.leaf_off[pr.x], bo = qs.off[pr.y];
    const uint32_t la = (uint32_t)(t.leaf_off[pr.x + 1] - ao), lb = (uint32_t)(qs.off[pr.y + 1] - bo);
    const uint64_t* A = t.leaf_hashes + ao;
    const uint64_t* B = qs.hashes + bo;
    if (InLds) {
      __syncthreads();
      for (uint32_t k = lane; k < la; k += 64) lds64[k] = A[k];
      for (uint32_t k = lane; k < lb; k += 64) lds64[la + k] = B[k];
      __syncthreads();
      A = lds64;
      B = lds64 + la;
    }
    // Leaf::similarity = leaf.compare(query) (the leaf's num truncates); Leaf::containment = count_common / |leaf|
    // (reference src/index/sbt.rs:546-577 over src/index.rs:131-161): an empty leaf gives NaN, which never passes
    const PairResult64 r = wave_compare_pair(A, la, B, lb, t.leaf_num[pr.x], lane);
    if (lane == 0) {
      const double v = containment ? (double)r.tot_c / (double)la
                                   : (double)r.common / (double)(r.size > 1 ? r.size : 1);
      if (v > threshold) hits[atomicAdd(hits_n, 1u)] = ((unsigned long long)pr.y << 32) | pr.x;
    }
  }
}

__global__ __launch_bounds__(256) void k_sbt_count_leaves(SbtDev t, const uint32_t* __restrict__ leaf_parent,
                                                          const uint32_t* __restrict__ sizes, const uint64_t* __restrict__ magic,
                                                          unsigned long long* __restrict__ tables) {
  const uint32_t leaf = blockIdx.x;
  const uint32_t p = leaf_parent[leaf];
  if (p == kChildNone) return;
  unsigned long long* tab = tables + (uint64_t)p * t.W;
  for (uint64_t i = t.leaf_off[leaf] + threadIdx.x; i < t.leaf_off[leaf + 1]; i += blockDim.x) {
    const uint64_t h = t.leaf_hashes[i];
    for (uint32_t tt = 0; tt < t.T; tt++) {
      const uint32_t bin = fastmod(h, magic[tt], sizes[tt]);
      atomicOr(&tab[t.woff[tt] + (bin >> 6)], 1ull << (bin & 63));
    }
  }
}

__global__ __launch_bounds__(256) void k_sbt_or_level(SbtDev t, uint32_t p0, uint64_t* __restrict__ tables) {
  const uint32_t p = p0 + blockIdx.x;
  uint64_t* dst = tables + (uint64_t)p * t.W;
  for (uint32_t w = threadIdx.x; w < t.W; w += blockDim.x) {
    uint64_t acc = dst[w];
    for (uint32_t c = 0; c < t.d; c++) {
      const uint32_t ch = t.child[(uint64_t)p * t.d + c];
      if (ch == kChildNone || (ch & kChildLeaf)) continue;
      acc |= tables[(uint64_t)ch * t.W + w];
    }
    dst[w] = acc;
  }
}

__global__ __launch_bounds__(64) void k_sbt_popcount(SbtDev t, uint64_t* __restrict__ occ) {
  const uint32_t node = blockIdx.x;
  const uint64_t* tab = t.tables + (uint64_t)node * t.W;
  uint64_t c = 0;
  for (uint32_t w = t.woff[0] + threadIdx.x; w < t.woff[1]; w += 64) c += __popcll(tab[w]);
  c = wave_sum_u64(c);
  if (threadIdx.x == 0) occ[node] = c;
}

// ---- Nodegraph::count / get over a batch
__global__ __launch_bounds__(256) void k_ng_minidx_init(const uint32_t* __restrict__ bins, uint64_t n, uint32_t T,
                                                        const uint64_t* __restrict__ bit_base, uint32_t* __restrict__ minidx) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    for (uint32_t t = 0; t < T; t++) minidx[bit_base[t] + bins[i * T + t]] = 0xffffffffu;
}
__global__ __launch_bounds__(256) void k_ng_minidx(const uint32_t* __restrict__ bins, uint64_t n, uint32_t T,
                                                   const uint64_t* __restrict__ bit_base, uint32_t* __restrict__ minidx) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    for (uint32_t t = 0; t < T; t++) atomicMin(&minidx[bit_base[t] + bins[i * T + t]], (uint32_t)i);
}
// hash i sets a new bit of table t iff the bit was clear before the batch and i is the first hash of the batch on it
__global__ __launch_bounds__(256) void k_ng_new(const uint32_t* __restrict__ bins, uint64_t n, uint32_t T,
                                                const uint64_t* __restrict__ bit_base, const uint32_t* __restrict__ minidx,
                                                const uint32_t* __restrict__ woff, const uint64_t* __restrict__ words,
                                                unsigned long long* __restrict__ counters, uint8_t* __restrict__ out_new) {
  unsigned long long nb = 0, nu = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t fresh = 0;
    for (uint32_t t = 0; t < T; t++) {
      const uint32_t bin = bins[i * T + t];
      const bool was = (words[woff[t] + (bin >> 6)] >> (bin & 63)) & 1;
      if (!was && minidx[bit_base[t] + bin] == (uint32_t)i) fresh++;
    }
    nb += fresh;
    nu += fresh ? 1 : 0;
    if (out_new) out_new[i] = fresh ? 1 : 0;
  }
  if (nb) atomicAdd(&counters[0], nb);
  if (nu) atomicAdd(&counters[1], nu);
}
__global__ __launch_bounds__(256) void k_ng_set(const uint32_t* __restrict__ bins, uint64_t n, uint32_t T,
                                                const uint32_t* __restrict__ woff, unsigned long long* __restrict__ words) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    for (uint32_t t = 0; t < T; t++) {
      const uint32_t bin = bins[i * T + t];
      atomicOr(&words[woff[t] + (bin >> 6)], 1ull << (bin & 63));
    }
}
__global__ __launch_bounds__(256) void k_ng_get(const uint32_t* __restrict__ bins, uint64_t n, uint32_t T,
                                                const uint32_t* __restrict__ woff, const uint64_t* __restrict__ words,
                                                uint8_t* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint8_t all = 1;
    for (uint32_t t = 0; t < T && all; t++) {
      const uint32_t bin = bins[i * T + t];
      all = (words[woff[t] + (bin >> 6)] >> (bin & 63)) & 1;
    }
    out[i] = all;
  }
}

uint32_t sbt_grid(uint64_t n) {
  const uint64_t g = (n + 255) / 256;
  return (uint32_t)(g < 4096 ? (g ? g : 1) : 4096);
}

}  // namespace

void launch_sbt_bins(const uint64_t* hashes, uint64_t n, const DeviceLayout& L, uint32_t* bins, hipStream_t s) {
  if (n == 0 || L.T == 0) return;
  hipLaunchKernelGGL(k_sbt_bins, dim3(sbt_grid(n)), dim3(256), 0, s, hashes, n, L.sizes, L.magic, L.T, bins);
  HIP_CHECK(hipGetLastError());
}

void launch_ng_count_many(const uint64_t* hashes, uint64_t n, const DeviceLayout& L, uint64_t* words, const uint32_t* bins,
                          uint32_t* minidx, const uint64_t* bit_base, unsigned long long* counters, uint8_t* out_new, hipStream_t s) {
  (void)hashes;
  if (n == 0) return;
  const dim3 g(sbt_grid(n)), b(256);
  hipLaunchKernelGGL(k_ng_minidx_init, g, b, 0, s, bins, n, L.T, bit_base, minidx);
  hipLaunchKernelGGL(k_ng_minidx, g, b, 0, s, bins, n, L.T, bit_base, minidx);
  hipLaunchKernelGGL(k_ng_new, g, b, 0, s, bins, n, L.T, bit_base, minidx, L.woff, words, counters, out_new);
  hipLaunchKernelGGL(k_ng_set, g, b, 0, s, bins, n, L.T, L.woff, (unsigned long long*)words);
  HIP_CHECK(hipGetLastError());
}

void launch_ng_get_many(const uint32_t* bins, uint64_t n, const DeviceLayout& L, const uint64_t* words, uint8_t* out, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_ng_get, dim3(sbt_grid(n)), dim3(256), 0, s, bins, n, L.T, L.woff, words, out);
  HIP_CHECK(hipGetLastError());
}

void launch_sbt_nodes(const SbtDev& t, const SbtQueries& q, const SbtLevel& lv, double threshold, bool containment,
                      bool lds, Device& dev, hipStream_t s) {
  if (lv.nn == 0) return;
  dev.prof_begin(s);
  if (lds)
    hipLaunchKernelGGL(k_sbt_nodes<true>, dim3(lv.nn), dim3(256), (size_t)t.W * 8, s, t, q, lv, threshold, containment ? 1u : 0u);
  else
    hipLaunchKernelGGL(k_sbt_nodes<false>, dim3(lv.nn), dim3(256), 0, s, t, q, lv, threshold, containment ? 1u : 0u);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("sbt_nodes", s);
}

void launch_sbt_fill(const SbtDev& t, const SbtLevel& lv, hipStream_t s) {
  if (lv.nn == 0) return;
  hipLaunchKernelGGL(k_sbt_fill, dim3(lv.nn), dim3(256), 0, s, t, lv);
  HIP_CHECK(hipGetLastError());
}

void launch_sbt_leaves(const SbtDev& t, const SbtQueries& q, const uint2* lp, const unsigned int* lp_n, uint32_t cap,
                       double threshold, bool containment, uint32_t max_leaf_len, uint32_t max_query_len,
                       unsigned long long* hits, unsigned int* hits_n, Device& dev, hipStream_t s) {
  if (cap == 0) return;
  const size_t need = ((size_t)max_leaf_len + max_query_len) * 8;
  const uint32_t grid = (uint32_t)dev.cu_count() * 32;
  dev.prof_begin(s);
  if (need <= 64 * 1024)
    hipLaunchKernelGGL(k_sbt_leaves<true>, dim3(grid), dim3(64), need ? need : 16, s, t, q, lp, lp_n, cap, threshold,
                       containment ? 1u : 0u, hits, hits_n);
  else
    hipLaunchKernelGGL(k_sbt_leaves<false>, dim3(grid), dim3(64), 16, s, t, q, lp, lp_n, cap, threshold,
                       containment ? 1u : 0u, hits, hits_n);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("sbt_leaves", s);
}

void launch_sbt_count_leaves(const SbtDev& t, uint32_t n_leaves, const uint32_t* leaf_parent, const DeviceLayout& L,
                             uint64_t* tables, hipStream_t s) {
  if (n_leaves == 0) return;
  hipLaunchKernelGGL(k_sbt_count_leaves, dim3(n_leaves), dim3(256), 0, s, t, leaf_parent, L.sizes, L.magic,
                     (unsigned long long*)tables);
  HIP_CHECK(hipGetLastError());
}

void launch_sbt_or_level(const SbtDev& t, uint32_t p0, uint32_t np, uint64_t* tables, hipStream_t s) {
  if (np == 0) return;
  hipLaunchKernelGGL(k_sbt_or_level, dim3(np), dim3(256), 0, s, t, p0, tables);
  HIP_CHECK(hipGetLastError());
}

void launch_sbt_popcount(const SbtDev& t, uint32_t n_nodes, uint64_t* occ, hipStream_t s) {
  if (n_nodes == 0) return;
  hipLaunchKernelGGL(k_sbt_popcount, dim3(n_nodes), dim3(64), 0, s, t, occ);
  HIP_CHECK(hipGetLastError());
}

}  // namespace smh
