// angular_kernels.hip -- gfx950 kernels of the angular similarity on abundances (include/sourmash_amd.h, "Angular
// similarity").  For two abundance-tracking sketches A and B:
//   norm2(A) = sum of a_h^2 over A, dot(A, B) = sum of a_h * b_h over the hashes both hold   (exact u64)
//   cosine = (double)dot / (sqrt((double)norm2A) * sqrt((double)norm2B)), clamped to 1; angular = 1 - 2 acos(cosine) / pi
//
//   k_angular_narrow   abundances of a device-resident sketch (u64 counts, or differences of u32 run starts) -> u32;
//                      a value of 2^32 or more lowers the error word
//   k_angular_norms    one wavefront per sketch: coalesced reads of the u32 abundances, the sum of squares in 64 bits with
//                      the carry watched; an overflow lowers the error word to the sketch's index (atomicMin: the LOWEST
//                      bad sketch is reported whichever wave gets there first)
//   k_angular_block    a pair, one against many, N x M: a workgroup owns one ROW sketch and a chunk of columns.  The row's
//                      hashes are staged in LDS as k_gather_hits stages its query -- whole (with the abundances beside
//                      them) up to kAngularSamples hashes, else every 2^s-th hash with the last s levels of the search in
//                      global memory; the lower end of the search window is carried from step to step.  Each wavefront
//                      takes columns of the chunk in turn, streams the column 64 elements per step (one coalesced read of
//                      hashes, one of abundances), looks each element up in the row, accumulates match ? a * b : 0 per lane
//                      and ends with one wave reduction; lane 0 writes dot, cosine and angular.  No atomics on the
//                      outputs, no cooperative launch, nothing is waited for.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "kernels.hpp"
#include "wave_ops.hpp"

namespace smh {
namespace {

constexpr uint32_t kAngularSamples = 4096;   // 32 KiB of hashes + 16 KiB of abundances: three workgroups per CU

__global__ __launch_bounds__(256) void k_angular_narrow(const uint64_t* __restrict__ counts, const uint32_t* __restrict__ starts,
                                                        uint32_t total, uint32_t n, uint32_t* __restrict__ out,
                                                        uint32_t* __restrict__ err, uint32_t err_value) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint64_t v;
  if (counts) v = counts[i];
  else v = (uint64_t)((i + 1 < n ? starts[i + 1] : total) - starts[i]);
  if (v >> 32) { atomicMin(err, err_value); v = 0xffffffffull; }
  out[i] = (uint32_t)v;
}

__global__ __launch_bounds__(256) void k_angular_norms(const uint32_t* __restrict__ abunds, const uint64_t* __restrict__ offsets,
                                                       uint32_t n, uint64_t* __restrict__ norm2, uint32_t* __restrict__ err) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const uint64_t lo = offsets[i], hi = offsets[i + 1];
  uint64_t sum = 0;
  bool carry = false;
  for (uint64_t t = lo + lane; t < hi; t += 64) {
    const uint64_t a = abunds[t];
    const uint64_t nx = sum + a * a;   // a < 2^32: the square fits
    carry |= nx < sum;
    sum = nx;
  }
  for (int off = 32; off; off >>= 1) {
    const uint64_t o = __shfl_xor(sum, off);
    const uint64_t nx = sum + o;
    carry |= nx < sum;
    sum = nx;
  }
  if (__ballot(carry) != 0ull) {
    if (lane == 0) { atomicMin(err, i); norm2[i] = ~0ull; }
    return;
  }
  if (lane == 0) norm2[i] = sum;
}

struct AngularArgs {
  const uint64_t* rh; const uint32_t* ra; const uint64_t* ro; const uint64_t* rn2; uint32_t n_rows;
  const uint64_t* ch; const uint32_t* ca; const uint64_t* co; const uint64_t* cn2; uint32_t n_cols;
  const uint64_t* prune;   // nullable: row-major n_rows x n_cols, 0 = the pair shares nothing
  uint32_t symmetric, chunk, n_chunks;
  uint64_t* dot; double* cosine; double* angular;
  unsigned long long* counters;   // [0] pairs walked, [1] pairs skipped
};

// the rules of include/sourmash_amd.h, in their order: IEEE conversions, sqrt, multiply, divide; nothing contracted
__device__ __forceinline__ void angular_finish(uint64_t dot, uint64_t n2a, uint64_t n2b, double* c_out, double* a_out) {
#pragma clang fp contract(off)
  double c = 0.0;
  if (dot != 0 && n2a != 0 && n2b != 0) {
    const double den = sqrt((double)n2a) * sqrt((double)n2b);
    c = (double)dot / den;
    if (c > 1.0) c = 1.0;
  }
  *c_out = c;
  double a;
  if (c == 0.0) a = 0.0;
  else if (c == 1.0) a = 1.0;
  else {
    const double t = 2.0 * acos(c);
    a = 1.0 - t / M_PI;
  }
  *a_out = a;
}

__device__ __forceinline__ void angular_write(const AngularArgs& p, uint32_t r, uint32_t c, uint64_t dot, double cs, double an) {
  const uint64_t at = (uint64_t)r * p.n_cols + c;
  if (p.dot) p.dot[at] = dot;
  if (p.cosine) p.cosine[at] = cs;
  if (p.angular) p.angular[at] = an;
}

__global__ __launch_bounds__(256) void k_angular_block(AngularArgs p) {
  __shared__ uint64_t samp[kAngularSamples];
  __shared__ uint32_t sab[kAngularSamples];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t r = blockIdx.x / p.n_chunks;
  const uint32_t c_lo = (blockIdx.x % p.n_chunks) * p.chunk;
  const uint32_t c_hi = min(c_lo + p.chunk, p.n_cols);
  const uint64_t ro = p.ro[r];
  const uint32_t lr = (uint32_t)(p.ro[r + 1] - ro);
  const uint64_t* __restrict__ Q = p.rh + ro;
  const uint32_t* __restrict__ QA = p.ra + ro;

  // is any pair of this workgroup walked at all?  (a pruned matrix is mostly workgroups that only write zeros)
  int mine = 0;
  for (uint32_t c = c_lo + tid; c < c_hi; c += 256) {
    if (p.symmetric && c <= r) continue;
    if (lr == 0 || p.co[c + 1] == p.co[c]) continue;
    if (p.prune && p.prune[(uint64_t)r * p.n_cols + c] == 0) continue;
    mine = 1;
  }
  const int any = __syncthreads_or(mine);

  uint32_t shift = 0;
  while ((((uint64_t)lr + (1ull << shift) - 1) >> shift) > kAngularSamples) shift++;
  const uint32_t m = (uint32_t)(((uint64_t)lr + (1ull << shift) - 1) >> shift);
  if (any) {
    for (uint32_t t = tid; t < m; t += 256) samp[t] = Q[(uint64_t)t << shift];
    if (shift == 0)
      for (uint32_t t = tid; t < m; t += 256) sab[t] = QA[t];
    __syncthreads();
  }

  const uint64_t n2r = p.rn2[r];
  uint32_t walked = 0, skipped = 0;
  for (uint32_t c = c_lo + w; c < c_hi; c += 4) {
    if (p.symmetric && c < r) continue;   // written by the wave that owns (c, r)
    const uint64_t n2c = p.cn2[c];
    if (p.symmetric && c == r) {
      if (lane == 0) angular_write(p, r, c, n2r, n2r ? 1.0 : 0.0, n2r ? 1.0 : 0.0);
      continue;
    }
    const uint64_t co = p.co[c];
    const uint32_t lc = (uint32_t)(p.co[c + 1] - co);
    const bool walk = lr != 0 && lc != 0 && (!p.prune || p.prune[(uint64_t)r * p.n_cols + c] != 0);
    uint64_t acc = 0;
    if (walk) {
      walked++;
      const uint64_t* __restrict__ B = p.ch + co;
      const uint32_t* __restrict__ BA = p.ca + co;
      uint32_t base = 0;   // every Q[< base] is smaller than this step's elements
      for (uint32_t i0 = 0; i0 < lc; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool ok = i < lc;
        const uint64_t b = ok ? B[i] : ~0ull;
        const uint32_t ab = ok ? BA[i] : 0u;
        // lo = number of samples below b; the samples in front of ceil(base / 2^s) are known to be
        uint32_t lo = (uint32_t)(((uint64_t)base + (1ull << shift) - 1) >> shift), len = m - lo;
        while (len > 0) {
          const uint32_t half = len >> 1, mid = lo + half;
          const bool lt = samp[mid] < b;
          lo = lt ? mid + 1 : lo;
          len = lt ? len - half - 1 : half;
        }
        uint32_t g = lo;
        bool match;
        uint32_t aa = 0;
        if (shift == 0) {
          match = ok && g < lr && samp[g] == b;
          if (match) aa = sab[g];
        } else {
          // sample lo - 1 < b <= sample lo: the lower bound lies in ((lo - 1) << s, lo << s], and not below base
          g = 0;
          if (lo != 0) {
            const uint32_t wlo = max(((lo - 1) << shift) + 1, base);
            const uint32_t whi = (uint32_t)min((uint64_t)lo << shift, (uint64_t)lr);
            g = wlo; len = whi - wlo;
            while (len > 0) {
              const uint32_t half = len >> 1, mid = g + half;
              const bool lt = Q[mid] < b;
              g = lt ? mid + 1 : g;
              len = lt ? len - half - 1 : half;
            }
          }
          match = ok && g < lr && Q[g] == b;
          if (match) aa = QA[g];
        }
        acc += match ? (uint64_t)aa * (uint64_t)ab : 0ull;   // no overflow: dot <= max(norm2) of two accepted sketches
        base = (uint32_t)__builtin_amdgcn_readlane((int)g, 63);
      }
      acc = wave_sum_u64(acc);
    } else {
      skipped++;
    }
    if (lane == 0) {
      double cs, an;
      angular_finish(acc, n2r, n2c, &cs, &an);
      angular_write(p, r, c, acc, cs, an);
      if (p.symmetric) angular_write(p, c, r, acc, cs, an);   // n_rows == n_cols; sqrt(a) * sqrt(b) commutes: the mirror is bit-equal
    }
  }
  if (lane == 0) {
    if (walked) atomicAdd(&p.counters[0], (unsigned long long)walked);
    if (skipped) atomicAdd(&p.counters[1], (unsigned long long)skipped);
  }
}

}  // namespace

void launch_angular_narrow(const uint64_t* counts, const uint32_t* starts, uint32_t total, uint32_t n, uint32_t* out,
                           uint32_t* err_dev, uint32_t err_value, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_angular_narrow, dim3((n + 255) / 256), dim3(256), 0, s, counts, starts, total, n, out, err_dev, err_value);
  HIP_CHECK(hipGetLastError());
}

void launch_angular_norms(const uint32_t* abunds, const uint64_t* offsets_dev, uint32_t n, uint64_t* norm2_dev, uint32_t* err_dev,
                          hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_angular_norms, dim3((n + 3) / 4), dim3(256), 0, s, abunds, offsets_dev, n, norm2_dev, err_dev);
  HIP_CHECK(hipGetLastError());
}

uint32_t angular_chunk(uint32_t n_rows, uint32_t n_cols) {
  // 256 columns (64 per wave) spread the staging of a row over many pairs; a block too small to fill the chip that way is
  // cut finer, down to one column per wave
  uint32_t chunk = 256;
  while (chunk > 4 && (uint64_t)n_rows * ((n_cols + chunk - 1) / chunk) < 1024) chunk >>= 1;
  return chunk;
}

void launch_angular_block(const AngularSet& rows, const AngularSet& cols, const uint64_t* prune_dev, bool symmetric,
                          const AngularOut& out, unsigned long long* counters_dev, Device& dev, hipStream_t s) {
  HIP_CHECK(hipMemsetAsync(counters_dev, 0, 16, s));
  if (rows.n == 0 || cols.n == 0) return;
  AngularArgs p;
  p.rh = rows.hashes; p.ra = rows.abunds; p.ro = rows.offsets; p.rn2 = rows.norm2; p.n_rows = rows.n;
  p.ch = cols.hashes; p.ca = cols.abunds; p.co = cols.offsets; p.cn2 = cols.norm2; p.n_cols = cols.n;
  p.prune = prune_dev;
  p.symmetric = symmetric ? 1u : 0u;
  p.chunk = angular_chunk(rows.n, cols.n);
  p.n_chunks = (cols.n + p.chunk - 1) / p.chunk;
  p.dot = out.dot; p.cosine = out.cosine; p.angular = out.angular;
  p.counters = counters_dev;
  const uint64_t grid = (uint64_t)rows.n * p.n_chunks;
  if (grid > 0x7fffffffull) throw_internal("angular: the block is too large for one launch");
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_angular_block, dim3((uint32_t)grid), dim3(256), 0, s, p);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("angular_block", s);
}

}  // namespace smh
