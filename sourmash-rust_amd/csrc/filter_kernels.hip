// filter_kernels.hip -- gfx950 kernels of filtering a resident index (include/sourmash_amd.h, "Filtering an index"; DESIGN.md
// 3.21): a verdict per resident hash, then an ordered compaction per node, with no host pass over hashes or nodes.
//
//   k_filter_flag     one workgroup per tile of kFilterTile CSR elements (element t counted from offsets[0]; a tile may span
//                     any number of nodes), tiles taken in a gridDim-stride loop.  Every lane evaluates the rule for its
//                     elements: membership in the operand by a search of its sorted hashes (sampled top in LDS, the last
//                     levels in global memory inside a 2^shift window: directory_lower_bound on the operand), the owner
//                     window by the same search on the hash directory and the length of the owner list, the abundance window
//                     on the element's own abundance.  The verdicts leave as a bit mask -- the ballot of a wave is one 64-bit
//                     word, stored by lane 0 with a plain vector store -- and the tile's survivor count.
//   k_filter_scan     the counts scanned in place, 64 bits wide (an index promises no total below 2^32): one workgroup walks
//                     them in blocks of 1024 with a carry.
//   k_filter_offsets  one lane per node boundary: the tile prefix at off[i] + the popcount of that tile's mask below off[i].
//   k_filter_emit     the same tiles again: a survivor's slot is the tile prefix + the popcount of the mask in front of it (the
//                     32 words of a tile scanned by one wave through shuffles).  It searches nothing -- except the operand
//                     again under OPERAND, for the survivors only, to fetch their abundance.
//
// A thread of flag / emit holds 8 elements: step s of the workgroup takes elements [256 s, 256 s + 256) of the tile, wave w of
// it the 64 from 64 w on, so mask word s * 4 + w of the tile is exactly that wave's ballot and bit t of the whole mask is
// element t.  Nothing spins, no workgroup waits for another, there is no atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "directory_probe.hpp"
#include "kernels.hpp"

namespace smh {
namespace {

constexpr uint32_t kSteps = kFilterTile / kFilterThreads;   // 8
constexpr uint32_t kWaves = kFilterThreads / 64;            // 4
constexpr uint32_t kScanThreads = 1024;
static_assert(kFilterTile % kFilterThreads == 0 && kFilterThreads % 64 == 0, "whole waves, whole steps");
static_assert(kSteps * kWaves == kFilterWords && kFilterWords <= 64, "a wave's ballot is a mask word; one wave scans a tile's words");

// m = ceil(n / 2^shift) <= kFilterSamples samples of the operand; shift == 0: all of it sits in LDS
void operand_sampling(uint32_t n, uint32_t* shift, uint32_t* m) {
  uint32_t sh = 0;
  while ((((uint64_t)n + (1ull << sh) - 1) >> sh) > kFilterSamples) sh++;
  *shift = sh;
  *m = (uint32_t)(((uint64_t)n + (1ull << sh) - 1) >> sh);
}

// the operand's hashes as the directory the probe's search takes (U and n_hashes are all it reads)
__device__ __forceinline__ MatchDirectory operand_view(const FilterPass& f) {
  MatchDirectory d;
  d.U = f.operand;
  d.n_hashes = f.n_operand;
  return d;
}

template <bool OPER, bool OWN>
__global__ __launch_bounds__(kFilterThreads) void k_filter_flag(const FilterPass f, uint32_t op_shift, uint32_t op_m, uint32_t dir_shift,
                                                                uint32_t dir_m, uint64_t tiles) {
  __shared__ uint64_t s_op[OPER ? kFilterSamples : 1];
  __shared__ uint64_t s_dir[OWN ? kMatchSamples : 1];
  __shared__ uint32_t part[kWaves];
  const MatchDirectory op = operand_view(f);
  if (OPER) directory_stage_samples(op, op_shift, op_m, s_op);
  if (OWN) directory_stage_samples(f.dir, dir_shift, dir_m, s_dir);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool window = f.abunds != nullptr && f.rule.abund_window();
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint32_t kept = 0;
#pragma unroll
    for (uint32_t s = 0; s < kSteps; s++) {
      const uint64_t t = tile * kFilterTile + (uint64_t)s * kFilterThreads + threadIdx.x;
      const bool ok = t < f.total;
      const uint64_t h = ok ? f.hashes[t] : 0;
      bool keep = ok;
      if (OPER) {
        const uint32_t pos = directory_lower_bound(op, s_op, op_shift, op_m, h, ok);
        const bool in = ok && pos < f.n_operand && f.operand[pos] == h;
        keep = keep && (in == (f.rule.operand_mode == kFilterKeepIn));
      }
      if (window) {
        const uint32_t a = ok ? f.abunds[t] : 0;
        keep = keep && a >= f.rule.min_abund && a <= f.rule.max_abund;
      }
      if (OWN) {
        const uint32_t g = directory_lower_bound(f.dir, s_dir, dir_shift, dir_m, h, ok);
        uint32_t owners = 0;
        if (ok && g < f.dir.n_hashes) {   // (a resident hash is in its index's directory: U[g] == h)
          uint32_t b, e;
          directory_owner_range(f.dir, g, &b, &e);
          owners = e - b;
        }
        keep = keep && owners >= f.rule.min_owners && owners <= f.rule.max_owners;
      }
      const uint64_t vote = __ballot(keep);
      if (lane == 0) f.mask[tile * kFilterWords + s * kWaves + wave] = vote;
      kept += (uint32_t)__popcll(vote);
    }
    if (lane == 0) part[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t sum = 0;
      for (uint32_t w = 0; w < kWaves; w++) sum += part[w];
      f.tile_at[tile] = sum;
    }
    __syncthreads();   // part is rewritten by the next trip
  }
}

// a[0 .. m) -> their exclusive prefix sums, a[m] = the total.  A block of 1024 counts adds up to at most 2^21, so the scan
// inside a block runs in 32 bits and only the carry is 64 bits wide.
__global__ __launch_bounds__(kScanThreads) void k_filter_scan(uint64_t* __restrict__ a, uint64_t m) {
  __shared__ uint32_t wsum[kScanThreads / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (uint64_t b = 0; b < m; b += kScanThreads) {
    const uint64_t i = b + threadIdx.x;
    const uint32_t v = i < m ? (uint32_t)a[i] : 0;
    uint32_t x = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)x, d);
      if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < kScanThreads / 64; w++) {
      const uint32_t c = wsum[w];
      before += w < wave ? c : 0;
      all += c;
    }
    if (i < m) a[i] = carry + before + (x - v);
    carry += all;
    __syncthreads();   // wsum is rewritten by the next block
  }
  if (threadIdx.x == 0) a[m] = carry;
}

__global__ __launch_bounds__(256) void k_filter_offsets(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ tile_at,
                                                        const uint64_t* __restrict__ off, uint32_t n, uint64_t* __restrict__ new_off) {
  const uint64_t base = off[0];
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * 256) {
    const uint64_t rel = off[i] - base, tile = rel / kFilterTile;
    const uint32_t within = (uint32_t)(rel % kFilterTile);
    uint64_t at = tile_at[tile];   // (rel == total on a tile boundary reads the last entry, the total, and no mask word)
    if (within) {
      const uint64_t* words = mask + tile * kFilterWords;
      for (uint32_t w = 0; w < (within >> 6); w++) at += (uint32_t)__popcll(words[w]);
      const uint32_t r = within & 63;
      if (r) at += (uint32_t)__popcll(words[within >> 6] & ((1ull << r) - 1));
    }
    new_off[i] = at;
  }
}

template <bool OPER>
__global__ __launch_bounds__(kFilterThreads) void k_filter_emit(const FilterPass f, uint32_t op_shift, uint32_t op_m, uint64_t tiles,
                                                                uint64_t* __restrict__ out_hashes, uint32_t* __restrict__ out_abunds) {
  __shared__ uint64_t s_op[OPER ? kFilterSamples : 1];
  __shared__ uint32_t wpre[kFilterWords];
  const MatchDirectory op = operand_view(f);
  if (OPER) directory_stage_samples(op, op_shift, op_m, s_op);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t start = f.tile_at[tile];
    if (f.tile_at[tile + 1] == start) continue;   // (uniform: a tile without survivors)
    const uint64_t* words = f.mask + tile * kFilterWords;
    if (wave == 0) {   // the survivors in front of every word of the tile
      const uint32_t c = lane < kFilterWords ? (uint32_t)__popcll(words[lane]) : 0;
      uint32_t x = c;
#pragma unroll
      for (uint32_t d = 1; d < kFilterWords; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, d);
        if (lane >= d) x += y;
      }
      if (lane < kFilterWords) wpre[lane] = x - c;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t s = 0; s < kSteps; s++) {
      const uint32_t wi = s * kWaves + wave;
      const uint64_t vote = words[wi];
      if ((vote >> lane) & 1ull) {   // (bits of elements beyond the total are 0)
        const uint64_t t = tile * kFilterTile + (uint64_t)s * kFilterThreads + threadIdx.x;
        const uint64_t slot = start + wpre[wi] + (uint32_t)__popcll(vote & below);
        const uint64_t h = f.hashes[t];
        out_hashes[slot] = h;
        if (out_abunds) {
          if (OPER) out_abunds[slot] = f.operand_abunds[directory_lower_bound(op, s_op, op_shift, op_m, h, true)];   // (kept: it is there)
          else out_abunds[slot] = f.abunds[t];
        }
      }
    }
    __syncthreads();   // wpre is rewritten by the next trip
  }
}

}  // namespace

void filter_geometry(uint32_t* tile, uint32_t* operand_samples, uint32_t* threads) {
  if (tile) *tile = kFilterTile;
  if (operand_samples) *operand_samples = kFilterSamples;
  if (threads) *threads = kFilterThreads;
}

void launch_filter_flag(const FilterPass& f, Device& dev, hipStream_t s) {
  const uint64_t tiles = filter_tiles(f.total);
  if (tiles == 0) return;
  const bool oper = f.rule.operand_mode != kFilterOperandNone, own = f.rule.owner_window();
  uint32_t op_shift = 0, op_m = 0, dir_shift = 0, dir_m = 0;
  if (oper) operand_sampling(f.n_operand, &op_shift, &op_m);
  if (own) directory_sampling(f.dir.n_hashes, &dir_shift, &dir_m);
  const dim3 grid(grid_for(tiles, 1, dev.grid_limit(), dev)), block(kFilterThreads);
  dev.prof_begin(s);
  if (oper && own) hipLaunchKernelGGL((k_filter_flag<true, true>), grid, block, 0, s, f, op_shift, op_m, dir_shift, dir_m, tiles);
  else if (oper) hipLaunchKernelGGL((k_filter_flag<true, false>), grid, block, 0, s, f, op_shift, op_m, dir_shift, dir_m, tiles);
  else if (own) hipLaunchKernelGGL((k_filter_flag<false, true>), grid, block, 0, s, f, op_shift, op_m, dir_shift, dir_m, tiles);
  else hipLaunchKernelGGL((k_filter_flag<false, false>), grid, block, 0, s, f, op_shift, op_m, dir_shift, dir_m, tiles);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("filter_flag", s);
}

void launch_filter_scan(uint64_t* tile_at, uint64_t tiles, hipStream_t s) {
  hipLaunchKernelGGL(k_filter_scan, dim3(1), dim3(kScanThreads), 0, s, tile_at, tiles);
  HIP_CHECK(hipGetLastError());
}

void launch_filter_offsets(const FilterPass& f, const uint64_t* offsets_dev, uint32_t n, uint64_t* new_off, Device& dev, hipStream_t s) {
  hipLaunchKernelGGL(k_filter_offsets, dim3(grid_for((uint64_t)n + 1, 256, dev.grid_limit(), dev)), dim3(256), 0, s, f.mask, f.tile_at,
                     offsets_dev, n, new_off);
  HIP_CHECK(hipGetLastError());
}

void launch_filter_emit(const FilterPass& f, uint64_t* out_hashes, uint32_t* out_abunds, Device& dev, hipStream_t s) {
  const uint64_t tiles = filter_tiles(f.total);
  if (tiles == 0) return;
  const bool oper = out_abunds != nullptr && f.rule.abund_out == kFilterAbundOperand;
  uint32_t op_shift = 0, op_m = 0;
  if (oper) operand_sampling(f.n_operand, &op_shift, &op_m);
  const dim3 grid(grid_for(tiles, 1, dev.grid_limit(), dev)), block(kFilterThreads);
  dev.prof_begin(s);
  if (oper) hipLaunchKernelGGL((k_filter_emit<true>), grid, block, 0, s, f, op_shift, op_m, tiles, out_hashes, out_abunds);
  else hipLaunchKernelGGL((k_filter_emit<false>), grid, block, 0, s, f, op_shift, op_m, tiles, out_hashes, out_abunds);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("filter_emit", s);
}

}  // namespace smh
