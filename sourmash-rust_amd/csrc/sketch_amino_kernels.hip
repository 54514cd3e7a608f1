// sketch_amino_kernels.hip -- gfx950 kernels for amino-acid input (smh_add_protein*, include/sourmash_amd.h "amino-acid
// input"; the reference hashes a protein sequence's windows as they are, src/lib.rs:275-276 and 289-300 without the
// translation):
//
//   k_amino_tiled<W>   every window of W <= 64 bytes of every record in one pass over LDS tiles, each byte upper-cased and
//                      taken through the sketch's alphabet (aa_map).
//   k_amino_generic    same contract for any window length, one lane per window start, byte-wise.
//
// MurmurHash3, the 32-bit halves (W2), the open digest and murmur_short are murmur_device.hpp's; the LDS stage and the
// record look-ups sketch_device.hpp's; the per-tile record table comes from with_tile_records (sketch_launch.hpp,
// sketch_kernels.hip).
// All arithmetic is 64-bit integer; results are bit-exact with the reference by construction
// and checked against oracle/ in tests/.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device.hpp"
#include "kernels.hpp"
#include "murmur_device.hpp"
#include "sketch_device.hpp"
#include "sketch_launch.hpp"

namespace smh {
namespace {

// The residue alphabets (include/sourmash_amd.h "alphabets"; HashParams::alphabet holds a Molecule): what an upper-cased
// byte is hashed as.  protein (and 0): itself.  Only the amino-acid kernels evaluate it, once per byte VALUE while they
// fill their table; the translated kernels read a composed codon table instead (kCodonAA).
__device__ __forceinline__ uint32_t aa_map(uint32_t alphabet, uint32_t c) {
  if (alphabet == 2u) {   // dayhoff
    switch (c) {
      case 'C': return 'a';
      case 'A': case 'G': case 'P': case 'S': case 'T': return 'b';
      case 'D': case 'E': case 'N': case 'Q': return 'c';
      case 'H': case 'K': case 'R': return 'd';
      case 'I': case 'L': case 'M': case 'V': return 'e';
      case 'F': case 'W': case 'Y': return 'f';
      case '*': return '*';
      default: return 'X';
    }
  }
  if (alphabet == 3u) {   // hp
    switch (c) {
      case 'A': case 'F': case 'G': case 'I': case 'L': case 'M': case 'P': case 'V': case 'W': case 'Y': return 'h';
      case 'N': case 'C': case 'S': case 'T': case 'D': case 'E': case 'R': case 'H': case 'K': case 'Q': return 'p';
      case '*': return '*';
      default: return 'X';
    }
  }
  return c;
}

// ---------------------------------------------------------------------------------
// amino-acid input (smh_add_protein*, include/sourmash_amd.h "amino-acid input"): every window of `win` bytes of every
// record, each byte upper-cased and taken through the sketch's alphabet; no strand, no translation, no byte is special.
//
// k_amino_tiled<W>: one pass.  A workgroup owns tiles of kAmTile window starts; the tile's bytes and a halo of win - 1 are
// read from HBM with aligned 16-byte loads, every byte is mapped ONCE through a 256-byte LDS table and the mapped dwords are
// staged in LDS so that dword 0 is the (4-byte aligned) dword holding the tile's first position.  A lane owns kAmRun = 16
// consecutive starts: it reads its 16-byte chunks back (ds_read_b128, lane stride 16 bytes), shifts out the sub-dword
// misalignment once and forms each window as a byte-shifted view of those registers (as hash_run does), hashes it with the
// dword murmur and tests the open digest.
// Record boundaries open no other path: the record starts that fall inside (T0, T0 + tile + win - 1) are walked by the
// workgroup -- record rec0 + 1 + tid + j * threads, rec0 from k_tile_records -- and marked in an LDS bit mask; every lane
// hashes every window, and the window at g is EMITTED iff no start bit lies in (g, g + win - 1] and g + win <= total.  Any
// number of starts per tile (1-byte records: more than threads) and zero-length records (bits set twice) are the same walk.
// W: compile-time for the usual window lengths, 0 = the run-time `win_rt` <= kAmMaxWin (windows then come from LDS
// with a run-time byte shift, and murmur's blocks are a loop).
constexpr int kAmThreads = 256;
constexpr int kAmRun = 16;
constexpr int kAmTile = kAmThreads * kAmRun;
constexpr int kAmMaxWin = 64;
constexpr int kAmTileDwords = 1056;                           // 3 + tile + 63 bytes of windows, + the whole dwords / chunks read past them
constexpr int kAmMaskWords = (kAmTile + kAmMaxWin) / 32 + 4;  // a lane reads four words from its run's
// run-time W: a window starts in dword (3 + tile - 1) / 4 at the latest and reads 1 + 4 * 5 dwords on; staging writes chunk 260 at the most
static_assert(kAmTileDwords > (3 + kAmTile - 1) / 4 + 21 && kAmTileDwords >= 4 * 261 && 4 * kAmTileDwords >= 16 * (kAmThreads - 1) + 48, "amino tile");

template <int W>
__global__ __launch_bounds__(kAmThreads) void k_amino_tiled(SeqBatch b, HashParams hp, CandSink sink, uint32_t win_rt, uint32_t stage_cap) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[kAmTileDwords];
  __shared__ uint32_t bmask[kAmMaskWords];
  __shared__ uint8_t lut[256];
  __shared__ uint64_t k2tab[W == 9 ? 256 : 1];
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const Stage stage{smem, reinterpret_cast<uint64_t*>(smem + 4), reinterpret_cast<uint64_t*>(smem + 4) + stage_cap, stage_cap};
  const uint32_t win = W ? (uint32_t)W : win_rt;
  const int tid = threadIdx.x;
  lut[tid] = (uint8_t)aa_map(hp.alphabet, upper((uint32_t)tid));   // 256 threads, 256 byte values
  if (W == 9) k2tab[tid] = hp.seed ^ mix_k2((uint64_t)tid) ^ (uint64_t)W;
  if (tid == 0) smem[0] = 0;
  __syncthreads();

  const uint32_t thr_hi1 = open_thr<false>(hp.thr);
  const uint64_t hi_pos = hp.range_hi < b.len ? hp.range_hi : b.len;      // window starts of this launch: [range_lo, hi_pos)
  const uint64_t ntiles = hi_pos > hp.range_lo ? (hi_pos - hp.range_lo + kAmTile - 1) / kAmTile : 0;
  const uintptr_t gend = ((uintptr_t)(b.seq + b.len) + 15) & ~(uintptr_t)15;
  const uint64_t clean_bits = win > 1 ? (~0ull >> (65 - win)) : 0ull;     // win - 1 low bits

  for (uint64_t tix = blockIdx.x; tix < ntiles; tix += gridDim.x) {
    // (every reader of the previous tile is behind the __syncthreads that stage_flush starts with)
    const uint64_t T0 = hp.range_lo + tix * kAmTile;
    const uintptr_t g0 = (uintptr_t)(b.seq + T0);
    const uintptr_t ga = g0 & ~(uintptr_t)15;
    const uint32_t m = (uint32_t)(g0 - ga), q = m >> 2, sh = m & 3u;
    const uint32_t nchunks = (m + (uint32_t)kAmTile + win - 1 + 15) >> 4;   // <= 261
    if (tid < kAmMaskWords) bmask[tid] = 0;
    for (uint32_t c = tid; c < nchunks; c += kAmThreads) {
      const uintptr_t addr = ga + ((uintptr_t)c << 4);
      uint4 v = make_uint4(0, 0, 0, 0);
      if (addr < gend) v = *reinterpret_cast<const uint4*>(addr);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int d = 0; d < 4; d++) {
        const uint32_t o = (uint32_t)lut[w[d] & 0xff] | ((uint32_t)lut[(w[d] >> 8) & 0xff] << 8) |
                           ((uint32_t)lut[(w[d] >> 16) & 0xff] << 16) | ((uint32_t)lut[w[d] >> 24] << 24);
        const uint32_t at = 4 * c + d;                    // < 1044 + 4
        if (at >= q) tile[at - q] = o;
      }
    }
    // record starts inside (T0, T0 + tile + win - 1): one bit each.  tile_rec is null for a batch of one record.
    if (b.tile_rec) {
      __syncthreads();                                    // the mask is zero
      const uint64_t lim = T0 + kAmTile + win - 1;
      for (uint64_t r = (uint64_t)b.tile_rec[tix].rec + 1 + tid; r < b.nrec; r += kAmThreads) {
        const uint64_t st = b.starts[r];
        if (st >= lim) break;
        const uint32_t o = (uint32_t)(st - T0);           // >= 1: rec is the LAST record that starts at or before T0
        atomicOr(&bmask[o >> 5], 1u << (o & 31));
      }
    }
    __syncthreads();

    const uint32_t o = (uint32_t)tid * kAmRun;
    const uint64_t p0 = T0 + o;
    if (p0 < hi_pos) {
      // start bits of positions (o & ~31) ... + 127, as two 64-bit halves
      const uint32_t* mw = bmask + (o >> 5);
      const uint64_t mlo = mw[0] | ((uint64_t)mw[1] << 32), mhi = mw[2] | ((uint64_t)mw[3] << 32);
      auto emit_ok = [&](uint32_t j) -> bool {             // the window at p0 + j lies inside one record and inside the launch
        const uint32_t bo = (o & 31u) + j + 1;             // 1 .. 32: bit of position p0 + j + 1
        const uint64_t v = (mlo >> bo) | (mhi << (64 - bo));
        const uint64_t g = p0 + j;
        return (v & clean_bits) == 0 && g < hi_pos && g + win <= b.len;
      };
      if constexpr (W != 0) {
        constexpr int ND = (kAmRun + W - 1 + 3) / 4;       // dwords holding the run's windows
        constexpr int NCH = (ND + 1 + 3) / 4;              // 16-byte chunks read: one dword more, for the sub-dword shift
        constexpr int NW = (W + 3) / 4;
        uint32_t X[4 * NCH], D[ND];
#pragma unroll
        for (int c = 0; c < NCH; c++) {
          const uint4 v = *reinterpret_cast<const uint4*>(tile + 4 * tid + 4 * c);
          X[4 * c] = v.x; X[4 * c + 1] = v.y; X[4 * c + 2] = v.z; X[4 * c + 3] = v.w;
        }
#pragma unroll
        for (int i = 0; i < ND; i++) D[i] = __builtin_amdgcn_alignbyte(X[i + 1], X[i], sh);
        W2 seedw{(uint32_t)hp.seed ^ (uint32_t)W, (uint32_t)(hp.seed >> 32)};
        asm volatile("" : "+v"(seedw.lo), "+v"(seedw.hi));
#pragma unroll
        for (int j = 0; j < kAmRun; j++) {
          uint32_t Wd[4] = {0, 0, 0, 0};
#pragma unroll
          for (int d = 0; d < NW; d++) {
            const int lo = d + (j >> 2);
            Wd[d] = (j & 3) ? __builtin_amdgcn_alignbyte(D[lo + 1 < ND ? lo + 1 : ND - 1], D[lo], j & 3) : D[lo];
            const int nb = W - 4 * d;
            if (nb < 4) Wd[d] &= (1u << (8 * nb)) - 1u;
          }
          W2 fa, fb;
          if (W < 16) {
            uint64_t h2r = 0;
            if (W == 9) h2r = k2tab[Wd[2] & 0xffu];
            murmur_short<W>(w2_mul(W2{Wd[0], Wd[1]}, kC1), W2{Wd[2], Wd[3]}, seedw, h2r, fa, fb);
          } else {                                         // sixteen bytes are one whole murmur block and no tail
            W2 h1{(uint32_t)hp.seed, (uint32_t)(hp.seed >> 32)}, h2 = h1;
            h1 = w2_xor(h1, w2_mul(w2_rotl(w2_mul(W2{Wd[0], Wd[1]}, kC1), 31), kC2));
            h1 = w2_mul5_add(w2_add(w2_rotl(h1, 27), h2), 0x52dce729ull);
            h2 = w2_xor(h2, w2_mul(w2_rotl(w2_mul(W2{Wd[2], Wd[3]}, kC2), 33), kC1));
            h2 = w2_mul5_add(w2_add(w2_rotl(h2, 31), h1), 0x38495ab5ull);
            h1.lo ^= 16u; h2.lo ^= 16u;
            w2_cross_add(h1, h2);
            fa = w2_fmix_pre(h1); fb = w2_fmix_pre(h2);
          }
          // (both closing multiplies for every window, then the filter on the products' high dwords: the filter on the
          // sum was measured here and is no gain by the project's rule -- DESIGN.md 3.11)
          const W2 pa = w2_mul(fa, kFmixC2), pb = w2_mul(fb, kFmixC2);
          if (pa.hi + pb.hi + 1u <= thr_hi1) {
            const uint64_t h = open_finish(pa, pb);
            if (h <= hp.thr && emit_ok((uint32_t)j)) stage_emit(stage, sink, h, hp.pos_base + p0 + j);
          }
        }
      } else {
        const int nblocks = (int)(win >> 4), tail = (int)(win & 15u);
        const uint64_t tmask_lo = tail >= 8 ? ~0ull : ((1ull << (8 * tail)) - 1ull);
        const uint64_t tmask_hi = tail > 8 ? ((1ull << (8 * (tail - 8))) - 1ull) : 0ull;
#pragma unroll 1
        for (uint32_t j = 0; j < (uint32_t)kAmRun; j++) {
          const uint32_t at = sh + o + j;                  // byte of the window's start in the LDS tile
          const uint32_t* src = tile + (at >> 2);
          const uint32_t bs = at & 3u;
          uint32_t prev = src[0];
          int ix = 1;
          auto next64 = [&]() -> uint64_t {
            const uint32_t n0 = src[ix], n1 = src[ix + 1];
            const uint32_t lo = __builtin_amdgcn_alignbyte(n0, prev, bs), hi = __builtin_amdgcn_alignbyte(n1, n0, bs);
            prev = n1; ix += 2;
            return lo | ((uint64_t)hi << 32);
          };
          uint64_t h1 = hp.seed, h2 = hp.seed;
          for (int blk = 0; blk < nblocks; blk++) {
            const uint64_t k1 = next64(), k2 = next64();
            mm3_block(h1, h2, k1, k2);
          }
          if (tail) {
            const uint64_t k1 = next64() & tmask_lo, k2 = next64() & tmask_hi;
            if (tail > 8) h2 ^= mix_k2(k2);
            h1 ^= mix_k1(k1);
          }
          const uint64_t h = mm3_finish(h1, h2, (uint64_t)win);
          if (h <= hp.thr && emit_ok(j)) stage_emit(stage, sink, h, hp.pos_base + p0 + j);
        }
      }
    }
    stage_flush(stage, sink, tid, kAmThreads);
  }
}

// any window length (the tiled kernel stops at kAmMaxWin): one lane per window start, byte-wise -- the part k_dna_generic
// plays in the DNA arm
__global__ __launch_bounds__(256) void k_amino_generic(SeqBatch b, HashParams hp, CandSink sink, uint32_t win) {
  __shared__ uint8_t lut[256];
  lut[threadIdx.x] = (uint8_t)aa_map(hp.alphabet, upper((uint32_t)threadIdx.x));
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t hi_pos = hp.range_hi < b.len ? hp.range_hi : b.len;
  for (uint64_t p = hp.range_lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < hi_pos; p += stride) {
    uint64_t end = b.len;
    if (b.starts) end = b.starts[find_record(b.starts, b.nrec, p) + 1];
    if (p + win > end || p + win < p) continue;
    Mm3Stream st(hp.seed);
    for (uint32_t i = 0; i < win; i++) st.push(lut[b.seq[p + i]]);
    const uint64_t h = st.finish();
    if (h <= hp.thr) emit(sink, h, hp.pos_base + p);
  }
}

}  // namespace

// ---------------------------------------------------------------------------------
// launchers

void amino_geometry(uint64_t total_len, uint32_t win, uint32_t* tile_positions, uint32_t* run) {
  (void)total_len;   // one geometry: a launch of any size cuts the same tiles
  const bool tiled = win >= 1 && win <= (uint32_t)kAmMaxWin;
  if (tile_positions) *tile_positions = tiled ? (uint32_t)kAmTile : 256u;
  if (run) *run = tiled ? (uint32_t)kAmRun : 1u;
}

void launch_amino_hash(const SeqBatch& b_in, uint32_t win, const HashParams& p, const CandSink& sink, Device& dev, hipStream_t s) {
  const uint64_t hi = p.range_hi < b_in.len ? p.range_hi : b_in.len;
  if (hi <= p.range_lo || win == 0) return;
  const uint64_t span = hi - p.range_lo;
  dev.prof_begin(s);
  if (win > (uint32_t)kAmMaxWin) {
    hipLaunchKernelGGL(k_amino_generic, dim3(sketch_grid(span, 256, dev.cu_count() * 16)), dim3(256), 0, s, b_in, p, sink, win);
    HIP_CHECK(hipGetLastError());
    dev.prof_end("amino_generic", s);
    return;
  }
  const uint64_t ntiles = (span + kAmTile - 1) / kAmTile;
  const SeqBatch b = with_tile_records(b_in, 0, p.range_lo, kAmTile, ntiles, dev, s);
  const int grid = (int)(ntiles < (uint64_t)dev.cu_count() * 8 ? ntiles : (uint64_t)dev.cu_count() * 8);
  long double expect = (long double)kAmTile * (((long double)p.thr + 1.0L) / 18446744073709551616.0L);
  uint32_t stage_cap = expect * 2.0L + 64.0L > 2048.0L ? 2048u : (uint32_t)(expect * 2.0L + 64.0L);
  if (stage_cap < 128) stage_cap = 128;
  const size_t lds = 16 + (size_t)stage_cap * 8 * (sink.pos ? 2 : 1);
#define SMH_AM(W_) hipLaunchKernelGGL(k_amino_tiled<W_>, dim3(grid), dim3(kAmThreads), lds, s, b, p, sink, win, stage_cap)
  if (win == 7) SMH_AM(7); else if (win == 9) SMH_AM(9); else if (win == 10) SMH_AM(10); else if (win == 16) SMH_AM(16); else SMH_AM(0);
#undef SMH_AM
  HIP_CHECK(hipGetLastError());
  dev.prof_end("amino_tiled", s);
}

}  // namespace smh
