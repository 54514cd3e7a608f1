// sigtext_kernels.hip -- a resident index -> the decimal text of its `mins` and `abundances` arrays and every node's md5, in
// HBM (the rules every byte follows are sigtext_core.hpp's, which a plain host build runs too).
//
//   1. k_sigtext_measure  per tile of kSigTextTile values: the decimal digits of its hashes and of its abundances, summed;
//   2. (scan)             the tile sums scanned in place, 64 bits wide (filter's scan), then k_sigtext_bounds, one lane per
//                         node boundary: the digit prefix at off[v] -- the tile's prefix plus a recount of the values of that
//                         tile in front of the boundary (fewer than a tile).  16 bytes per node go to the host, which lays
//                         the text out (sigtext.cpp);
//   3. k_sigtext_emit     per tile the digits again, a block scan for every value's place, the tile's bytes -- a comma slot
//                         and the digits per value -- built in LDS, then copied to the text segment by segment (a segment: the
//                         part of one node's array that lies in the tile, contiguous in the text): 16-byte stores on the
//                         destination's own 16-byte grid, single bytes only in front of and behind it;
//      k_sigtext_place    the skeleton pieces, byte by byte (a few hundred bytes per node);
//   4. k_sigtext_md5      one wave per node: 64 values per step formatted into LDS without separators, every complete
//                         64-byte block compressed by all lanes alike, the remainder carried; RFC 1321's padding at the end;
//      k_sigtext_hex      the digests as 32 hex digits into their places in the text.
// Every kernel walks its items in a gridDim-stride loop (grid_for).  Every store to the text is checked against its length.
#include "kernels.hpp"
#include "sigtext_core.hpp"
#include "wave_ops.hpp"

namespace smh {

namespace {

using namespace sigtext;

constexpr uint32_t kThreads = kSigTextThreads;
constexpr uint32_t kTile = kSigTextTile;
constexpr uint32_t kPer = kTile / kThreads;          // values per thread, consecutive
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kSlot = kMaxDigits64 + 1;         // the most bytes a value takes in a tile's image: a comma slot and its digits
constexpr uint32_t kImageWords = (kTile * kSlot + 3) / 4 + 2;   // (the copy reads whole words: two of slack)
static_assert(kTile % kThreads == 0 && kThreads % 64 == 0, "whole waves, whole steps");
static_assert(kTile * kSlot < 65536 && kTile < 65536, "the scan packs bytes and segments into 16 bits each");

__device__ __forceinline__ uint32_t digits_any(uint64_t v) { return digits_u64(v); }
__device__ __forceinline__ uint32_t digits_any(uint32_t v) { return digits_u32(v); }
__device__ __forceinline__ uint32_t format_any(uint64_t v, uint8_t* out) { return format_u64(v, out); }
__device__ __forceinline__ uint32_t format_any(uint32_t v, uint8_t* out) { return format_u32(v, out); }

__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, d);
    if (lane >= d) x += y;
  }
  return x;
}

// ---------------------------------------------------------------------------------------------------------------
// pass 1

__global__ __launch_bounds__(kThreads) void k_sigtext_measure(const uint64_t* __restrict__ hashes, const uint32_t* __restrict__ abunds,
                                                              uint64_t total, uint64_t tiles, uint64_t* __restrict__ tile_h,
                                                              uint64_t* __restrict__ tile_a) {
  __shared__ uint32_t acc[2];
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    if (threadIdx.x < 2) acc[threadIdx.x] = 0;
    __syncthreads();
    uint32_t dh = 0, da = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) {
      const uint64_t i = tile * kTile + (uint64_t)k * kThreads + threadIdx.x;
      if (i < total) {
        dh += digits_u64(hashes[i]);
        if (abunds) da += digits_u32(abunds[i]);
      }
    }
    dh = wave_sum(dh);
    da = wave_sum(da);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&acc[0], dh); atomicAdd(&acc[1], da); }
    __syncthreads();
    if (threadIdx.x == 0) { tile_h[tile] = acc[0]; if (tile_a) tile_a[tile] = acc[1]; }
    __syncthreads();   // acc is zeroed by the next trip
  }
}

// pass 2, behind the scan: the digit prefix at every node boundary.  off: n + 1 entries; values are counted from off[0].
__global__ __launch_bounds__(256) void k_sigtext_bounds(const uint64_t* __restrict__ hashes, const uint32_t* __restrict__ abunds,
                                                        const uint64_t* __restrict__ tile_h, const uint64_t* __restrict__ tile_a,
                                                        const uint64_t* __restrict__ off, uint32_t n, uint64_t* __restrict__ node_h,
                                                        uint64_t* __restrict__ node_a) {
  const uint64_t base = off[0];
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * 256) {
    const uint64_t rel = off[i] - base, tile = rel / kTile;
    const uint32_t within = (uint32_t)(rel % kTile);
    uint64_t h = tile_h[tile], a = abunds ? tile_a[tile] : 0;   // (rel == total on a tile boundary reads the last entry, the total)
    for (uint32_t j = 0; j < within; j++) {
      h += digits_u64(hashes[tile * kTile + j]);
      if (abunds) a += digits_u32(abunds[tile * kTile + j]);
    }
    node_h[i] = h;
    if (abunds) node_a[i] = a;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// pass 3

__device__ __forceinline__ uint32_t node_of(const uint64_t* off, uint64_t base, uint32_t n, uint64_t i) {   // the last v < n with off[v] - base <= i
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] - base <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// image[b, e) -> text[dst, dst + e - b), by the lanes who, who + stride, ...: whole 16-byte chunks of the destination's
// address grid as one store each, the bytes in front of the first and behind the last whole chunk one by one.
__device__ __forceinline__ void copy_segment(const uint32_t* image, uint32_t b, uint32_t e, uint8_t* text, uint64_t dst, uint64_t text_len,
                                             uint32_t who, uint32_t stride) {
  const uint32_t len = e - b;
  if (dst > text_len || len > text_len - dst) return;   // (a disagreement of the passes must not write outside)
  uint8_t* d = text + dst;
  const uint32_t lead = (uint32_t)((uintptr_t)d & 15);
  const uint32_t chunks = (lead + len + 15) / 16;
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(image);
  for (uint32_t c = who; c < chunks; c += stride) {
    const int32_t lo = (int32_t)(c * 16) - (int32_t)lead;   // the chunk's first byte, counted from the segment's
    if (lo >= 0 && (uint32_t)lo + 16 <= len) {
      const uint32_t at = b + (uint32_t)lo, sh = 8 * (at & 3);
      const uint32_t* w = image + (at >> 2);
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
      uint4 q;
      q.x = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
      q.y = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
      q.z = (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh);
      q.w = (uint32_t)((((uint64_t)w4 << 32) | w3) >> sh);
      *reinterpret_cast<uint4*>(d + lo) = q;
    } else {
      for (int32_t k = 0; k < 16; k++) {
        const int32_t p = lo + k;
        if (p >= 0 && (uint32_t)p < len) d[p] = bytes[b + (uint32_t)p];
      }
    }
  }
}

// values: total of them, counted from off[0] (the pointer stands at that element).  tile_pre: the scanned tile sums; node_pre[v]:
// the digit prefix at off[v]; node_at[v]: where the inside of node v's array begins in the text.
template <class V>
__global__ __launch_bounds__(kThreads) void k_sigtext_emit(const V* __restrict__ values, uint64_t total, uint64_t tiles,
                                                           const uint64_t* __restrict__ tile_pre, const uint64_t* __restrict__ off, uint32_t n,
                                                           const uint64_t* __restrict__ node_pre, const uint64_t* __restrict__ node_at,
                                                           uint8_t* __restrict__ text, uint64_t text_len) {
  __shared__ uint32_t image[kImageWords];
  __shared__ uint32_t seg_lds[kTile + 1];
  __shared__ uint64_t seg_txt[kTile];
  __shared__ uint32_t wsum[kWaves];
  uint8_t* bytes = reinterpret_cast<uint8_t*>(image);
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t base = off[0];
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t t0 = tile * kTile, first = t0 + (uint64_t)tid * kPer;
    V val[kPer];
    uint32_t dg[kPer], node[kPer];
    bool opens[kPer];
    uint32_t mine = 0;   // bytes in the low half, segments in the high half
    uint32_t v = first < total ? node_of(off, base, n, first) : 0;
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) {
      const uint64_t i = first + k;
      val[k] = 0; dg[k] = 0; node[k] = 0; opens[k] = false;
      if (i < total) {
        while (off[v + 1] - base <= i) v++;   // (i < total = off[n] - base: ends with v < n)
        val[k] = values[i];
        dg[k] = digits_any(val[k]);
        node[k] = v;
        opens[k] = i == off[v] - base;
        mine += (dg[k] + 1) + ((opens[k] || i == t0) ? 1u << 16 : 0u);
      }
    }
    const uint32_t incl = wave_scan_incl(mine, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; w++) {
      const uint32_t c = wsum[w];
      before += w < wave ? c : 0;
      all += c;
    }
    uint32_t at = (before + incl - mine) & 0xffff, seg = (before + incl - mine) >> 16;
    const uint32_t image_len = all & 0xffff, segs = all >> 16;
    const uint64_t pre0 = tile_pre[tile];
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) {
      const uint64_t i = first + k;
      if (i < total) {
        bytes[at] = ',';
        format_any(val[k], bytes + at + 1);
        if (opens[k] || i == t0) {
          const uint32_t u = node[k];
          // the value's first digit stands at node_at + (digits of the node in front of it) + (values of the node in front of it)
          const uint64_t digit_at = node_at[u] + (pre0 + (at - (uint32_t)(i - t0)) - node_pre[u]) + (i - (off[u] - base));
          seg_lds[seg] = opens[k] ? at + 1 : at;          // a node's first value has no comma: its slot is left out
          seg_txt[seg] = opens[k] ? digit_at : digit_at - 1;
          seg++;
        }
        at += dg[k] + 1;
      }
    }
    if (tid == 0) seg_lds[segs] = image_len + 1;   // (a segment ends in front of the comma slot of the next one's first value)
    __syncthreads();
    if (segs < kWaves) {
      for (uint32_t s = 0; s < segs; s++) copy_segment(image, seg_lds[s], seg_lds[s + 1] - 1, text, seg_txt[s], text_len, tid, kThreads);
    } else {
      for (uint32_t s = wave; s < segs; s += kWaves) copy_segment(image, seg_lds[s], seg_lds[s + 1] - 1, text, seg_txt[s], text_len, lane, 64);
    }
    __syncthreads();   // the image and the segments are rewritten by the next trip
  }
}

// piece p = skeleton[piece_src[p], piece_src[p + 1]) -> text[piece_dst[p] ..)
__global__ __launch_bounds__(256) void k_sigtext_place(const uint8_t* __restrict__ skeleton, uint64_t skeleton_len,
                                                       const uint64_t* __restrict__ piece_src, const uint64_t* __restrict__ piece_dst,
                                                       uint64_t pieces, uint8_t* __restrict__ text, uint64_t text_len) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < skeleton_len; i += (uint64_t)gridDim.x * 256) {
    uint64_t lo = 0, hi = pieces;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (piece_src[mid] <= i) lo = mid; else hi = mid;
    }
    const uint64_t at = piece_dst[lo] + (i - piece_src[lo]);
    if (at < text_len) text[at] = skeleton[i];
  }
}

__global__ __launch_bounds__(256) void k_sigtext_hex(const uint8_t* __restrict__ digests, const uint64_t* __restrict__ md5_at, uint32_t n,
                                                     uint8_t* __restrict__ text, uint64_t text_len) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < (uint64_t)n * 32; i += (uint64_t)gridDim.x * 256) {
    const uint64_t v = i >> 5;
    const uint32_t c = (uint32_t)(i & 31), b = digests[v * 16 + (c >> 1)];
    const uint64_t at = md5_at[v] + c;
    if (at < text_len) text[at] = hex_digit((c & 1) ? (b & 15u) : (b >> 4));
  }
}

// ---------------------------------------------------------------------------------------------------------------
// pass 4: one wave per workgroup, one node per trip

constexpr uint32_t kMd5Step = kSigTextMd5Step;
constexpr uint32_t kMd5Words = (64 + kMd5Step * kMaxDigits64) / 4;   // what a step can hold: a carried remainder and its values
static_assert(kMd5Step == 64, "a step is one value per lane");

__global__ __launch_bounds__(64) void k_sigtext_md5(const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ off, uint32_t n,
                                                    const uint32_t* __restrict__ ksizes, uint8_t* __restrict__ digests) {
  __shared__ uint32_t buf[kMd5Words];
  uint8_t* bytes = reinterpret_cast<uint8_t*>(buf);
  const uint32_t lane = threadIdx.x;
  const uint64_t base = off[0];
  for (uint64_t v = blockIdx.x; v < n; v += gridDim.x) {
    const uint64_t begin = off[v] - base, count = off[v + 1] - off[v];
    Md5State st;
    md5_init(st);
    const uint32_t ks = ksizes[v];
    uint32_t fill = digits_u32(ks);
    uint64_t total_bytes = fill;
    if (lane == 0) format_u32(ks, bytes);
    for (uint64_t s0 = 0; s0 < count; s0 += kMd5Step) {
      const uint64_t i = s0 + lane;
      const bool have = i < count;
      const uint64_t val = have ? hashes[begin + i] : 0;
      const uint32_t d = have ? digits_u64(val) : 0;
      const uint32_t incl = wave_scan_incl(d, lane);
      const uint32_t sum = (uint32_t)__shfl((int)incl, 63, 64);
      if (have) format_u64(val, bytes + fill + (incl - d));
      __syncthreads();
      const uint32_t end = fill + sum, blocks = end / 64, rem = end % 64;
      for (uint32_t b = 0; b < blocks; b++) md5_block(st, buf + b * 16);
      const uint8_t keep = lane < rem ? bytes[blocks * 64 + lane] : 0;
      __syncthreads();
      if (lane < rem) bytes[lane] = keep;
      fill = rem;
      total_bytes += sum;
    }
    __syncthreads();
    md5_finish(st, bytes, fill, total_bytes);
    if (lane < 16) digests[v * 16 + lane] = (uint8_t)md5_digest_byte(st, lane);
    __syncthreads();   // the buffer is rewritten by the next trip
  }
}

}  // namespace

void sigtext_geometry(uint32_t* values_per_tile, uint32_t* threads, uint32_t* md5_values_per_step) {
  if (values_per_tile) *values_per_tile = kTile;
  if (threads) *threads = kThreads;
  if (md5_values_per_step) *md5_values_per_step = kMd5Step;
}

void launch_sigtext_measure(const SigTextPass& p, Device& dev, hipStream_t s) {
  const uint64_t tiles = sigtext_tiles(p.total);
  dev.prof_begin(s);
  if (tiles) {
    hipLaunchKernelGGL(k_sigtext_measure, dim3(grid_for(tiles, 1, dev.grid_limit(), dev)), dim3(kThreads), 0, s, p.hashes, p.abunds, p.total, tiles,
                       p.tile_h, p.tile_a);
    HIP_CHECK(hipGetLastError());
  }
  dev.prof_end("sigtext_measure", s);
  dev.prof_begin(s);
  launch_filter_scan(p.tile_h, tiles, s);
  if (p.abunds) launch_filter_scan(p.tile_a, tiles, s);
  hipLaunchKernelGGL(k_sigtext_bounds, dim3(grid_for((uint64_t)p.n + 1, 256, dev.grid_limit(), dev)), dim3(256), 0, s, p.hashes, p.abunds, p.tile_h,
                     p.tile_a, p.off, p.n, p.node_h, p.node_a);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("sigtext_scan", s);
}

void launch_sigtext_emit(const SigTextPass& p, const SigTextPlace& w, Device& dev, hipStream_t s) {
  const uint64_t tiles = sigtext_tiles(p.total);
  dev.prof_begin(s);
  if (w.skeleton_len) {
    hipLaunchKernelGGL(k_sigtext_place, dim3(grid_for(w.skeleton_len, 256, dev.grid_limit(), dev)), dim3(256), 0, s, w.skeleton, w.skeleton_len,
                       w.piece_src, w.piece_dst, w.pieces, w.text, w.text_len);
    HIP_CHECK(hipGetLastError());
  }
  if (tiles) {
    const dim3 grid(grid_for(tiles, 1, dev.grid_limit(), dev));
    hipLaunchKernelGGL(k_sigtext_emit<uint64_t>, grid, dim3(kThreads), 0, s, p.hashes, p.total, tiles, p.tile_h, p.off, p.n, p.node_h, w.mins_at,
                       w.text, w.text_len);
    if (p.abunds)
      hipLaunchKernelGGL(k_sigtext_emit<uint32_t>, grid, dim3(kThreads), 0, s, p.abunds, p.total, tiles, p.tile_a, p.off, p.n, p.node_a,
                         w.abunds_at, w.text, w.text_len);
    HIP_CHECK(hipGetLastError());
  }
  if (p.n) {   // behind the pieces: the digits replace their placeholders
    hipLaunchKernelGGL(k_sigtext_hex, dim3(grid_for((uint64_t)p.n * 32, 256, dev.grid_limit(), dev)), dim3(256), 0, s, w.digests, w.md5_at, p.n,
                       w.text, w.text_len);
    HIP_CHECK(hipGetLastError());
  }
  dev.prof_end("sigtext_emit", s);
}

void launch_sigtext_md5(const uint64_t* hashes, const uint64_t* off, uint32_t n, const uint32_t* ksizes, uint8_t* digests, Device& dev,
                        hipStream_t s) {
  if (n == 0) return;
  dev.prof_begin(s);
  // a chain is latency-bound: eight waves per SIMD, each its own node
  hipLaunchKernelGGL(k_sigtext_md5, dim3(grid_for(n, 1, dev.grid_limit() * 4, dev)), dim3(64), 0, s, hashes, off, n, ksizes, digests);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("sigtext_md5", s);
}

}  // namespace smh
