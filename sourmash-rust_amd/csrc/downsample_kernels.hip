// downsample_kernels.hip -- cutting scaled sketches at a smaller max_hash without leaving HBM.
//
// A scaled sketch is the ascending set of its hashes <= max_hash, so the cut is a prefix of every segment of a CSR:
//   k_downsample_bounds  one wave per sketch: the number of hashes <= max_hash (upper bound, unsigned, inclusive)
//   k_downsample_copy    one workgroup per tile of kDownsampleTile OUTPUT elements: the kept prefixes to their new place,
//                        hashes and (when given) u32 abundances in one launch
//   k_downsample_cut     the same bound for one device-resident sketch, with the total its run starts end at
#include "kernels.hpp"

namespace smh {

namespace {

// The number of elements of the ascending seg[0 .. len) that are <= mx, found by the whole wave: every round probes the last
// element of 64 equal pieces (one 8-byte load per lane), the ballot says which piece holds the boundary.  log64(len) rounds
// of one dependent load each, against log2(len) for a thread of its own.  Every lane returns the answer.
__device__ __forceinline__ uint64_t wave_upper_bound(const uint64_t* __restrict__ seg, uint64_t len, uint64_t mx, uint32_t lane) {
  uint64_t lo = 0, hi = len;   // the answer lies in [lo, hi]; elements in front of lo are <= mx, those from hi on are > mx
  while (lo < hi) {
    const uint64_t step = (hi - lo + 63) >> 6;
    const uint64_t idx = lo + (uint64_t)(lane + 1) * step - 1;
    const bool le = idx < hi && seg[idx] <= mx;
    const uint32_t c = (uint32_t)__popcll(__ballot(le));   // ascending: the lanes that answer true are a prefix
    const uint64_t piece = lo + (uint64_t)c * step;         // pieces in front of this one lie wholly at or below mx
    const uint64_t probe = piece + step - 1;                // the probe of the boundary's piece: > mx when it exists
    lo = piece < hi ? piece : hi;
    if (probe < hi) hi = probe;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_downsample_bounds(const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ offsets,
                                                           uint32_t n, uint64_t mx, uint32_t* __restrict__ kept) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t sk = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sk >= n) return;   // (whole waves leave: the ballot below sees every lane of those that stay)
  const uint64_t b = offsets[sk], e = offsets[sk + 1];
  const uint64_t k = wave_upper_bound(hashes + b, e - b, mx, lane);
  if (lane == 0) kept[sk] = (uint32_t)k;
}

__global__ __launch_bounds__(64) void k_downsample_cut(const uint64_t* __restrict__ uniq, uint64_t n, const uint32_t* __restrict__ starts,
                                                       uint64_t total, uint64_t mx, uint64_t* __restrict__ out2) {
  const uint64_t cut = wave_upper_bound(uniq, n, mx, threadIdx.x);
  if (threadIdx.x == 0) {
    out2[0] = cut;
    out2[1] = starts ? (cut < n ? (uint64_t)starts[cut] : total) : cut;   // run starts: the kept runs end where run `cut` begins
  }
}

constexpr uint32_t kSegCap = 1024;   // segments of a tile whose offsets are staged in LDS (2 x 8 KiB + 16 bytes)

// the last s in [0, m) with off[s] <= o (off[0] <= o is the caller's)
__device__ __forceinline__ uint32_t seg_of(const uint64_t* off, uint32_t m, uint64_t o) {
  uint32_t lo = 0, hi = m;   // off[lo] <= o; off[hi] > o or hi == m
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= o) lo = mid; else hi = mid;
  }
  return lo;
}

struct CopyParams {
  const uint64_t* hashes;
  const uint32_t* abunds;        // nullable
  const uint64_t* src_off;       // n + 1 (device): where every segment begins in `hashes`
  const uint64_t* new_off;       // n + 1 (device): where its kept prefix begins in the output; new_off[0] == 0
  uint64_t* out_hashes;
  uint32_t* out_abunds;
  uint64_t total;                // new_off[n]
  uint32_t n;
  uint32_t wide_stores;          // both outputs are 16-byte aligned
};

// Output element o of the tile belongs to the segment s with new_off[s] <= o < new_off[s + 1] and comes from
// src_off[s] + (o - new_off[s]).  The workgroup finds the first and the last segment of its tile once, stages the offsets of
// those segments in LDS (a tile crossing more than kSegCap segments -- long stretches of tiny or empty sketches -- reads
// them from global memory instead), then every lane takes groups of four consecutive output elements: one search for the
// group's first element, a walk over segment ends for the other three.  Stores are 16 bytes wide whenever the outputs are
// aligned; a group that lies in one segment loads 16 bytes wide when its source has the destination's parity and 8 (hashes)
// or 4 (abundances) bytes wide otherwise.
__global__ __launch_bounds__(kDownsampleThreads) void k_downsample_copy(const CopyParams p) {
  __shared__ uint64_t s_new[kSegCap + 1], s_src[kSegCap + 1];
  __shared__ uint32_t s_first, s_last;
  const uint64_t lo = (uint64_t)blockIdx.x * kDownsampleTile;
  const uint64_t hi = lo + kDownsampleTile < p.total ? lo + kDownsampleTile : p.total;
  if (lo >= hi) return;
  if (threadIdx.x == 0) s_first = seg_of(p.new_off, p.n, lo);
  if (threadIdx.x == 64) s_last = seg_of(p.new_off, p.n, hi - 1);
  __syncthreads();
  const uint32_t first = s_first, m = s_last - first + 1;   // segments first .. first + m - 1 hold the tile
  const bool staged = m <= kSegCap;
  if (staged) {
    for (uint32_t i = threadIdx.x; i <= m; i += kDownsampleThreads) { s_new[i] = p.new_off[first + i]; s_src[i] = p.src_off[first + i]; }
    __syncthreads();
  }
  const uint64_t* noff = staged ? s_new : p.new_off + first;
  const uint64_t* soff = staged ? s_src : p.src_off + first;
  for (uint64_t o = lo + 4ull * threadIdx.x; o < hi; o += 4ull * kDownsampleThreads) {
    uint32_t s = seg_of(noff, m, o);
    const uint32_t cnt = hi - o < 4 ? (uint32_t)(hi - o) : 4u;
    uint64_t src = soff[s] + (o - noff[s]);
    uint64_t h[4] = {0, 0, 0, 0};
    uint32_t a[4] = {0, 0, 0, 0};
    if (cnt == 4 && o + 3 < noff[s + 1]) {   // the group lies inside one segment
      const uint64_t* hp = p.hashes + src;
      if (((uintptr_t)hp & 15) == 0) {
        const ulonglong2 v0 = *reinterpret_cast<const ulonglong2*>(hp), v1 = *reinterpret_cast<const ulonglong2*>(hp + 2);
        h[0] = v0.x; h[1] = v0.y; h[2] = v1.x; h[3] = v1.y;
      } else {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(hp + 1);
        h[0] = hp[0]; h[1] = v.x; h[2] = v.y; h[3] = hp[3];
      }
      if (p.abunds) {
        const uint32_t* ap = p.abunds + src;
        if (((uintptr_t)ap & 15) == 0) {
          const uint4 v = *reinterpret_cast<const uint4*>(ap);
          a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
        } else {
          a[0] = ap[0]; a[1] = ap[1]; a[2] = ap[2]; a[3] = ap[3];
        }
      }
    } else {
      for (uint32_t k = 0; k < cnt; k++) {
        const uint64_t ok = o + k;
        while (ok >= noff[s + 1]) s++;   // ends (and empty segments) crossed; ok < hi <= noff[m] stops it inside the tile's segments
        src = soff[s] + (ok - noff[s]);
        h[k] = p.hashes[src];
        if (p.abunds) a[k] = p.abunds[src];
      }
    }
    if (cnt == 4 && p.wide_stores) {
      ulonglong2 w0, w1;
      w0.x = h[0]; w0.y = h[1]; w1.x = h[2]; w1.y = h[3];
      *reinterpret_cast<ulonglong2*>(p.out_hashes + o) = w0;
      *reinterpret_cast<ulonglong2*>(p.out_hashes + o + 2) = w1;
      if (p.abunds) *reinterpret_cast<uint4*>(p.out_abunds + o) = make_uint4(a[0], a[1], a[2], a[3]);
    } else {
      for (uint32_t k = 0; k < cnt; k++) {
        p.out_hashes[o + k] = h[k];
        if (p.abunds) p.out_abunds[o + k] = a[k];
      }
    }
  }
}

}  // namespace

void downsample_geometry(uint32_t* tile_elems, uint32_t* threads) {
  if (tile_elems) *tile_elems = kDownsampleTile;
  if (threads) *threads = kDownsampleThreads;
}

void launch_downsample_bounds(const uint64_t* hashes, const uint64_t* offsets_dev, uint32_t n, uint64_t max_hash, uint32_t* kept_dev,
                              Device& dev, hipStream_t s) {
  if (n == 0) return;
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_downsample_bounds, dim3((n + 3) / 4), dim3(256), 0, s, hashes, offsets_dev, n, max_hash, kept_dev);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("downsample_bounds", s);
}

void launch_downsample_copy(const uint64_t* hashes, const uint32_t* abunds, const uint64_t* src_offsets_dev,
                            const uint64_t* new_offsets_dev, uint32_t n, uint64_t total, uint64_t* out_hashes, uint32_t* out_abunds,
                            Device& dev, hipStream_t s) {
  if (n == 0 || total == 0) return;
  const uint64_t grid = (total + kDownsampleTile - 1) / kDownsampleTile;
  if (grid > 0x7fffffffull) throw_internal("downsample: the kept hashes are too many for one launch");
  CopyParams p;
  p.hashes = hashes; p.abunds = abunds; p.src_off = src_offsets_dev; p.new_off = new_offsets_dev;
  p.out_hashes = out_hashes; p.out_abunds = abunds ? out_abunds : nullptr; p.total = total; p.n = n;
  p.wide_stores = (((uintptr_t)out_hashes | (abunds ? (uintptr_t)out_abunds : 0)) & 15) == 0;
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_downsample_copy, dim3((uint32_t)grid), dim3(kDownsampleThreads), 0, s, p);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("downsample_copy", s);
}

void launch_downsample_cut(const uint64_t* uniq, uint64_t n, const uint32_t* starts, uint64_t total, uint64_t max_hash, uint64_t* out2_dev,
                           hipStream_t s) {
  hipLaunchKernelGGL(k_downsample_cut, dim3(1), dim3(64), 0, s, uniq, n, starts, total, max_hash, out2_dev);
  HIP_CHECK(hipGetLastError());
}

}  // namespace smh
