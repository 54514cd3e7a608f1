// sketch_protein_kernels.hip -- gfx950 kernels for the six-frame protein arm of KmerMinHash::add_sequence
// (reference src/lib.rs:275-302):
//
//   k_protein_fused<W> protein arm in one pass: translation + hashing of both strands' windows, no residue
//                      buffer (lib.rs:275-302, 691-793); k_protein_positions rewrites candidate positions.
//   k_translate        six-frame translation into a residue buffer, unknown codons marked (lib.rs:277-301,
//   k_hash_windows     779-793) + every window of `win` residues, skipping dropped codons (lib.rs:289-300):
//                      the two-pass path for batches with non-ASCII bytes, partial ranges, other window lengths.
//   k_spliced_windows  the fused kernel's rare windows that skip dropped codons, walked like the reference (lib.rs:779-793).
//
// MurmurHash3, the 32-bit halves (W2), the open digest and murmur_short are murmur_device.hpp's; the LDS stage and the
// record look-ups sketch_device.hpp's; the per-tile record table comes from with_tile_records (sketch_launch.hpp,
// sketch_kernels.hip).
// All arithmetic is 64-bit integer; results are bit-exact with the reference by construction
// and checked against oracle/ in tests/.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "device.hpp"
#include "kernels.hpp"
#include "murmur_device.hpp"
#include "sketch_device.hpp"
#include "sketch_launch.hpp"

namespace smh {
namespace {

// ---------------------------------------------------------------------------------
// protein arm, phase 1: translate.  Residue buffer layout: for record r, segments
// 6r+0..6r+5 = (frame 0 fwd, frame 0 rc, frame 1 fwd, frame 1 rc, frame 2 fwd, frame 2 rc),
// the order the reference walks them; an unknown codon becomes kDropped.
constexpr uint32_t kDropped = 0xFFu;
// (three tables of 64: the codon table as it is, and composed with the dayhoff and the hp map -- codon_table(alphabet)
// picks one, so a codon look-up costs the same in every alphabet)
__constant__ char kCodonAA[3 * 64 + 1] =
    "FFLLSSSSYY**CC*W" "LLLLPPPPHHQQRRRR" "IIIMTTTTNNKKSSRR" "VVVVAAAADDEEGGGG"   // T,C,A,G order
    "ffeebbbbff**aa*f" "eeeebbbbddccdddd" "eeeebbbbccddbbdd" "eeeebbbbccccbbbb"   // dayhoff
    "hhhhpppphh**pp*h" "hhhhhhhhpppppppp" "hhhhpppppppppppp" "hhhhhhhhpppphhhh";  // hp
__device__ __forceinline__ const char* codon_table(uint32_t alphabet) { return kCodonAA + (alphabet >= 2u ? 64u * (alphabet - 1u) : 0u); }

__device__ __forceinline__ int tcag(uint32_t c) {
  return c == 'T' ? 0 : c == 'C' ? 1 : c == 'A' ? 2 : c == 'G' ? 3 : -1;
}
__device__ __forceinline__ uint32_t comp_upper(uint32_t c) {
  return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}
// str::from_utf8 on a 3-byte chunk (reference src/lib.rs:787 unwraps it)
__device__ __forceinline__ bool utf8_ok3(uint32_t a, uint32_t c, uint32_t d) {
  auto cont = [](uint32_t v) { return v >= 0x80 && v <= 0xBF; };
  auto lead2 = [](uint32_t v) { return v >= 0xC2 && v <= 0xDF; };
  if (a < 0x80) {
    if (c < 0x80) return d < 0x80;
    return lead2(c) && cont(d);
  }
  if (lead2(a)) return cont(c) && d < 0x80;
  if (a == 0xE0) return c >= 0xA0 && c <= 0xBF && cont(d);
  if (a == 0xED) return c >= 0x80 && c <= 0x9F && cont(d);
  if (a >= 0xE1 && a <= 0xEF) return cont(c) && cont(d);
  return false;
}

// Six-frame translation in ONE read of the sequence.  Every base position p of a record is the first
// base of exactly one forward codon (frame p mod 3, residue p/3) and the last-read base of exactly one
// reverse-complement codon (frame (len-1-p) mod 3), so one lane per base position produces both
// from the five bytes p-2 .. p+2, served from an LDS tile that the workgroup loaded with coalesced
// 16-byte reads.  Segment order in the residue buffer: reference src/lib.rs:280-300.
constexpr int kTrThreads = 256;
// 12 consecutive bases per lane: every frame gets 4 consecutive residues from a lane (forward:
// ascending, reverse: descending), written as ONE unaligned 4-byte store; consecutive lanes write
// consecutive dwords of the same frame.  (One byte store per residue -- 25 G of them for 12.5 GB
// of DNA -- is what bounded the first version, not HBM.)
constexpr int kTrPerThread = 12;
constexpr int kTrTile = kTrThreads * kTrPerThread;  // bases per workgroup tile

__global__ __launch_bounds__(kTrThreads) void k_translate(SeqBatch b, const uint64_t* __restrict__ seg_off,
                                                          uint32_t nseg, uint32_t ksize, uint32_t alphabet, uint8_t* __restrict__ res,
                                                          uint32_t* __restrict__ bad_utf8) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTrTile + 64];   // raw bytes (only the UTF-8 check reads them)
  __shared__ __attribute__((aligned(16))) uint8_t code[kTrTile + 64];   // T0 C1 A2 G3 (complement = ^2), 0x80 = not a base
  __shared__ uint8_t lut_code[256];
  __shared__ uint8_t lut_aa[64];
  const int tid = threadIdx.x;
  {
    // byte -> base code, case-insensitive (the reference upper-cases first, src/lib.rs:253-256)
    const uint32_t c = (uint32_t)tid, u = upper(c);
    const int t = tcag(u);
    lut_code[tid] = t < 0 ? 0x80u : (uint8_t)t;
    if (tid < 64) lut_aa[tid] = (uint8_t)codon_table(alphabet)[tid];   // the codon table composed with the alphabet
  }
  const uint64_t ntiles = (b.len + kTrTile - 1) / kTrTile;
  const uintptr_t gend = ((uintptr_t)(b.seq + b.len) + 15) & ~(uintptr_t)15;
  // a workgroup owns a CONTIGUOUS run of tiles: the record holding the tile start is found by
  // binary search once and then walked forward (a search per lane per tile is a chain of ~14
  // dependent loads for 10^4 records -- it used to dominate this bandwidth-bound kernel)
  const uint64_t per_wg = (ntiles + gridDim.x - 1) / gridDim.x;
  const uint64_t t_begin = (uint64_t)blockIdx.x * per_wg;
  const uint64_t t_end = t_begin + per_wg < ntiles ? t_begin + per_wg : ntiles;
  uint32_t rec0 = 0;
  if (b.starts && t_begin < t_end) rec0 = find_record(b.starts, b.nrec, t_begin * kTrTile);
  for (uint64_t tix = t_begin; tix < t_end; tix++) {
    const uint64_t T0 = tix * kTrTile;
    if (b.starts)
      while (rec0 + 1 < b.nrec && T0 >= b.starts[rec0 + 1]) rec0++;   // uniform
    // tile bytes [T0 - 16, T0 + kTrTile + 16) relative to an aligned base (a halo of 2 each side is needed)
    const uintptr_t g0 = (uintptr_t)(b.seq + T0);
    const uintptr_t ga = (g0 & ~(uintptr_t)15) - 16;
    const uint32_t m = (uint32_t)(g0 - ga);  // 16..31: offset of position T0 inside the tile
    __syncthreads();
    for (uint32_t c = tid; c < (kTrTile + 64) / 16; c += kTrThreads) {
      const uintptr_t addr = ga + ((uintptr_t)c << 4);
      uint4 v = make_uint4(0, 0, 0, 0);
      if (addr >= ((uintptr_t)b.seq & ~(uintptr_t)15) && addr < gend) v = *reinterpret_cast<const uint4*>(addr);
      *reinterpret_cast<uint4*>(tile + (c << 4)) = v;
      uint32_t w[4] = {v.x, v.y, v.z, v.w}, o[4];
#pragma unroll
      for (int d = 0; d < 4; d++)
        o[d] = (uint32_t)lut_code[w[d] & 0xff] | ((uint32_t)lut_code[(w[d] >> 8) & 0xff] << 8) |
               ((uint32_t)lut_code[(w[d] >> 16) & 0xff] << 16) | ((uint32_t)lut_code[w[d] >> 24] << 24);
      *reinterpret_cast<uint4*>(code + (c << 4)) = make_uint4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();
    // record of the lane's first position; lanes then step forward (records are walked in order)
    uint32_t rec = 0;
    uint64_t rs = 0, re = b.len;
    const uint64_t pfirst = T0 + (uint64_t)tid * kTrPerThread;
    if (b.starts && pfirst < b.len) {
      rec = rec0;
      // many tiny records inside one tile: search instead of walking
      if (rec0 + 8 < b.nrec && pfirst >= b.starts[rec0 + 8]) rec = find_record(b.starts, b.nrec, pfirst);
      rs = b.starts[rec]; re = b.starts[rec + 1];
    }
    // fast path: the lane's 12 bases and their 2-base halos lie inside one record that is long enough
    bool packed = false;
    if (pfirst < b.len) {
      while (pfirst >= re) { rec++; rs = b.starts[rec]; re = b.starts[rec + 1]; }
      const uint64_t rl = re - rs, o = pfirst - rs;
      packed = rl >= ksize && o >= 2 && o + kTrPerThread + 2 <= rl;
      if (packed) {
        const uint32_t x0 = m + (uint32_t)(pfirst - T0);
        uint32_t k[kTrPerThread + 4];   // codes of bases pfirst-2 .. pfirst+13
        uint32_t anybad = 0;
#pragma unroll
        for (int i = 0; i < kTrPerThread + 4; i++) { k[i] = code[x0 - 2 + i]; anybad |= k[i]; }
        if (anybad & 0x80u) packed = false;   // a non-base byte: the per-base path sorts out dropped codons / UTF-8
        if (packed) {
          const uint32_t of = (uint32_t)(o % 3);
          const uint64_t back0 = rl - 1 - o;          // reverse index of the lane's first base
          const uint32_t bf = (uint32_t)(back0 % 3);
#pragma unroll
          for (int c = 0; c < 3; c++) {
            // forward codons starting at bases c, c+3, c+6, c+9 of the run: frame (o+c)%3, residues (o+c)/3 ..+3
            uint32_t v = 0;
#pragma unroll
            for (int t = 0; t < 4; t++) {
              const int i = 2 + c + 3 * t;
              v |= (uint32_t)lut_aa[(k[i] << 4) | (k[i + 1] << 2) | k[i + 2]] << (8 * t);
            }
            uint32_t fr = of + c; fr = fr >= 3 ? fr - 3 : fr;
            __builtin_memcpy(res + seg_off[6 * rec + 2 * fr] + (o + c) / 3, &v, 4);
            // reverse codons whose first base is base c, c+3, c+6, c+9: reverse index back0-c-3t,
            // frame (back0-c)%3, residues (back0-c)/3 down to (back0-c)/3-3
            uint32_t w = 0;
#pragma unroll
            for (int t = 0; t < 4; t++) {
              const int i = 2 + c + 3 * t;
              w |= (uint32_t)lut_aa[((k[i] << 4) | (k[i - 1] << 2) | k[i - 2]) ^ 0x2a] << (8 * (3 - t));
            }
            uint32_t br = bf + 3 - c; br = br >= 3 ? br - 3 : br;
            __builtin_memcpy(res + seg_off[6 * rec + 2 * br + 1] + (back0 - c) / 3 - 3, &w, 4);
          }
        }
      }
    }
    if (!packed) {
    for (int q = 0; q < kTrPerThread; q++) {
      const uint64_t p = pfirst + q;
      if (p >= b.len) break;
      while (p >= re) { rec++; rs = b.starts[rec]; re = b.starts[rec + 1]; }
      const uint64_t rl = re - rs, o = p - rs;
      if (rl < ksize) continue;  // reference src/lib.rs:257: shorter records add nothing
      const uint32_t x = m + (uint32_t)(p - T0);
      const uint32_t k0 = code[x];
      // forward codon starting at o
      if (o + 2 < rl) {
        const uint32_t k1 = code[x + 1], k2 = code[x + 2];
        const uint32_t seg = 6 * rec + 2 * (uint32_t)(o % 3);
        const uint32_t bad = (k0 | k1 | k2) & 0x80u;
        if (bad) {
          const uint32_t c0 = upper(tile[x]), c1 = upper(tile[x + 1]), c2 = upper(tile[x + 2]);
          if (((c0 | c1 | c2) & 0x80u) && !utf8_ok3(c0, c1, c2)) atomicOr(&bad_utf8[seg], 1u);
        }
        res[seg_off[seg] + o / 3] = bad ? (uint8_t)kDropped : lut_aa[(k0 << 4) | (k1 << 2) | k2];
      }
      // reverse-complement codon whose first base is the complement of position o
      if (o >= 2) {
        const uint32_t k1 = code[x - 1], k2 = code[x - 2];
        const uint64_t back = rl - 1 - o;
        const uint32_t seg = 6 * rec + 2 * (uint32_t)(back % 3) + 1;
        const uint32_t bad = (k0 | k1 | k2) & 0x80u;
        if (bad) {
          const uint32_t d0 = comp_upper(upper(tile[x])), d1 = comp_upper(upper(tile[x - 1])), d2 = comp_upper(upper(tile[x - 2]));
          if (((d0 | d1 | d2) & 0x80u) && !utf8_ok3(d0, d1, d2)) atomicOr(&bad_utf8[seg], 1u);
        }
        res[seg_off[seg] + back / 3] = bad ? (uint8_t)kDropped : lut_aa[(((k0 << 4) | (k1 << 2) | k2)) ^ 0x2a];
      }
    }
    }
  }
}

// ---------------------------------------------------------------------------------
// protein arm, fused: translation and hashing in ONE pass over the DNA, no residue buffer.
//
// A window of `W` residues of any of the six frames is the translation of 3W consecutive bases --
// read forward, or read backward and complemented.  Every start position `a` of a record with
// a + 3W <= length carries exactly one forward window (frame a mod 3) and exactly one
// reverse-complement window, so the arm is the DNA kernel's walk with k = 3W and TWO hashes per
// position instead of a canonical choice.  A lane keeps, for each of the three reading frames that
// pass through its run, the last W residues of the forward translation and of the reverse-complement
// translation (byte strings in registers).  Each base completes one codon: its six digit bits index a
// 64-entry LDS table that holds the codon's residue and the residue of its reverse complement; the
// forward string of that frame shifts down a byte and takes the new residue on top, the
// reverse-complement string shifts up and takes it at the bottom (reference src/lib.rs:280-300 reads
// revcomp(sequence) forward, which is the record backward), and both strings are hashed
// (MurmurHash3 x64_128 of W <= 16 bytes: no full block, k1 and k2 straight from the registers).
//
// That covers every window whose 3W bases are all ACGT inside one record.  Windows that SKIP dropped
// codons (to_aa drops a codon holding anything else and splices its neighbours together, quirk Q8)
// are rare: the lane notices that a span is not clean with the same group test as the DNA kernel
// and puts its start position on a list; k_spliced_windows, a second tiny launch, walks the bytes
// of those spans in global memory exactly like the reference.  (A routine called from inside the
// hashing kernel needs a stack, and a kernel with a stack costs ~110 us more PER LAUNCH on this
// stack -- more than hashing a 5 Mbp genome.)  A byte >= 0x80 anywhere in the batch (where
// str::from_utf8 could panic, src/lib.rs:787) or a full list raises `high_flag`: the host then
// discards this launch and takes the two-pass path (k_translate + k_hash_windows), which
// reproduces the panic semantics and has no limits.
//
// Candidate positions are residue indices of the six-frame layout (segment 6r + 2*frame + strand),
// the order the reference walks them; seg_off is that layout's segment table.

// The hashing kernel reports a candidate's position as (a << 1 | strand): the first base of the
// window's span in the batch, strand 1 = reverse complement -- no table look-up on its emit path (a
// dependent global load there, taken by one lane in five hundred, stalls the whole wave).  When the
// caller wants positions (order-dependent sketch modes, grouped batches) this kernel rewrites them
// as residue indices of the six-frame layout, the order the reference walks the windows in.
__global__ __launch_bounds__(256) void k_protein_positions(uint64_t* __restrict__ pos, const unsigned long long* __restrict__ count,
                                                           uint64_t capacity, const uint64_t* __restrict__ starts, uint32_t nrec,
                                                           uint64_t batch_len, const uint64_t* __restrict__ seg_off, uint32_t kb,
                                                           uint64_t pos_base) {
  const uint64_t n = *count < capacity ? *count : capacity;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t code = pos[i], a = code >> 1;
    uint32_t rec = 0;
    uint64_t rs = 0, re = batch_len;
    if (starts) { rec = find_record(starts, nrec, a); rs = starts[rec]; re = starts[rec + 1]; }
    const uint64_t a_rel = a - rs, len = re - rs;
    uint64_t g;
    if ((code & 1) == 0) {
      g = seg_off[6 * (uint64_t)rec + 2 * (a_rel % 3)] + a_rel / 3;
    } else {
      const uint64_t rcidx = len - a_rel - kb;              // index, in revcomp(record), of the window's first base
      g = seg_off[6 * (uint64_t)rec + 2 * (rcidx % 3) + 1] + rcidx / 3;
    }
    pos[i] = pos_base + g;
  }
}

__device__ __forceinline__ int dna_digit(uint32_t c) {      // A0 C1 G2 T3 (either case), -1 otherwise
  const uint32_t u = c & 0xDFu;
  return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : -1;
}
__device__ __forceinline__ uint32_t aa_of_digits(const char* table, int d0, int d1, int d2) {   // table: codon_table(alphabet)
  // kCodonAA is indexed in T C A G order
  const int t[4] = {2, 1, 3, 0};
  return (uint32_t)(uint8_t)table[16 * t[d0] + 4 * t[d1] + t[d2]];
}

// The two windows that START (forward) / whose first residue lies (reverse complement) in the span
// [a, a + 3W) when that span is not all-ACGT-in-one-record: walk codon by codon, dropping codons
// that hold anything but ACGT, like to_aa + windows() of the reference (src/lib.rs:779-793, 289-300).
// (everything by value: a reference parameter of a non-inlined function would force the caller's
// kernel arguments into scratch memory)
// the windows that START at base `a` with dropped codons spliced out (one forward, one reverse complement), straight
// to the global sink
__device__ __forceinline__ void spliced_windows(const SeqBatch& b, const HashParams& hp, const CandSink& sink, uint32_t win, uint64_t a) {
  const uint32_t kb = 3 * win;
  const char* table = codon_table(hp.alphabet);
  uint32_t rec = 0;
  uint64_t rs = 0, re = b.len;
  if (b.starts) { rec = find_record(b.starts, b.nrec, a); rs = b.starts[rec]; re = b.starts[rec + 1]; }
  const uint64_t len = re - rs;
  if (len < hp.ksize || a < rs || a >= re) return;          // reference src/lib.rs:257
  // forward: first residue = codon [a, a+3) of frame a_rel % 3, then the following codons of that frame
  {
    const uint32_t f = (uint32_t)((a - rs) % 3);
    const uint64_t fend = rs + f + 3 * ((len - f) / 3);     // end of the frame's translated extent
    Mm3Stream st(hp.seed);
    uint32_t got = 0;
    for (uint64_t c = a; c + 3 <= fend && got < win; c += 3) {
      const int d0 = dna_digit(b.seq[c]), d1 = dna_digit(b.seq[c + 1]), d2 = dna_digit(b.seq[c + 2]);
      if (d0 < 0 || d1 < 0 || d2 < 0) { if (c == a) break; continue; }   // a window starts at a KEPT residue
      st.push(aa_of_digits(table, d0, d1, d2));
      got++;
    }
    if (got == win) {
      const uint64_t h = st.finish();
      if (h <= hp.thr) emit(sink, h, a << 1);
    }
  }
  // reverse complement: first residue = the codon read backward from base a + 3W - 1
  if (a + kb <= re) {
    const uint64_t e = a + kb - 1;
    Mm3Stream st(hp.seed);
    uint32_t got = 0;
    for (uint64_t c = e; c >= rs + 2 && got < win; c -= 3) {
      const int d0 = dna_digit(b.seq[c]), d1 = dna_digit(b.seq[c - 1]), d2 = dna_digit(b.seq[c - 2]);
      if (d0 < 0 || d1 < 0 || d2 < 0) { if (c == e) break; if (c < 3) break; continue; }
      st.push(aa_of_digits(table, 3 - d0, 3 - d1, 3 - d2));
      got++;
      if (c < 3) break;                                     // (c -= 3 must not wrap)
    }
    if (got == win) {
      const uint64_t h = st.finish();
      if (h <= hp.thr) emit(sink, h, (a << 1) | 1u);
    }
  }
}

constexpr uint32_t kSplicedCap = 1u << 20;   // spans a launch may set aside (more: the two-pass path)
__global__ __launch_bounds__(256) void k_spliced_windows(SeqBatch b, HashParams hp, CandSink sink, uint32_t win,
                                                         const uint64_t* __restrict__ list, const uint32_t* __restrict__ count) {
  const uint32_t n = *count < kSplicedCap ? *count : kSplicedCap;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) spliced_windows(b, hp, sink, win, list[i]);
}

// byte BYTE of x, shifted left by SH, in one sub-dword-addressed instruction (full rate; see k_dna_rolling, sketch_dna_kernels.hip)
template <int SH, int BYTE>
__device__ __forceinline__ uint32_t byte_shl(uint32_t x) {
  static_assert(SH == 3 && BYTE >= 0 && BYTE < 4, "byte_shl");
  uint32_t r;
#define SMH_BSHL(SH_, B_) asm("v_lshlrev_b32_sdwa %0, " #SH_ ", %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_" #B_ : "=v"(r) : "v"(x))
  if (BYTE == 0) SMH_BSHL(3, 0); else if (BYTE == 1) SMH_BSHL(3, 1); else if (BYTE == 2) SMH_BSHL(3, 2); else SMH_BSHL(3, 3);
#undef SMH_BSHL
  return r;
}

#ifndef SMH_PF_MINW
#define SMH_PF_MINW 4
#endif
#ifndef SMH_PF_LOGR
#define SMH_PF_LOGR 7
#endif
template <int W, int THREADS>
__global__ __launch_bounds__(THREADS, SMH_PF_MINW) void k_protein_fused(SeqBatch b, HashParams hp, CandSink sink, int logR,
                                                                          uint32_t stage_cap, uint32_t* __restrict__ high_flag,
                                                                          uint64_t* __restrict__ slow_list, uint32_t* __restrict__ slow_count) {
  constexpr int KB = 3 * W;                          // bases per window
  constexpr int ND = (W + 3) / 4;                    // dwords of a residue string
  // static LDS: codon tables -- codon number (its first base's digit lowest) -> (residue of the reverse complement) * c1 |
  // W == 9: seed ^ mix_k2(residue) ^ W | residue + residue of the reverse complement << 8 -- as three arrays of 8-byte
  // entries read with ONE offset register (32-byte records would put every look-up of a wave on eight banks), and
  // seed ^ mix_k2(byte) ^ W of any byte (W == 9: the reverse strand's k2 is a residue met eight codons earlier)
  __shared__ uint64_t ctab[3 * 64];
  __shared__ uint64_t k2tab[W == 9 ? 256 : 1];
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint32_t* st_ctl = smem;
  uint64_t* st_hash = reinterpret_cast<uint64_t*>(st_ctl + 4);
  uint64_t* st_pos = st_hash + stage_cap;
  uint32_t* tile = reinterpret_cast<uint32_t*>(st_pos + (sink.pos ? stage_cap : 0));
  const Stage stage{st_ctl, st_hash, st_pos, stage_cap};

  const int tid0 = threadIdx.x;
  const uint32_t R = 1u << logR;
  const uint64_t TILE = (uint64_t)THREADS << logR;
  const bool multi = b.starts != nullptr;
  if (tid0 < 64) {
    const int d0 = tid0 & 3, d1 = (tid0 >> 2) & 3, d2 = (tid0 >> 4) & 3;
    const char* table = codon_table(hp.alphabet);
    const uint32_t af = aa_of_digits(table, d0, d1, d2), ar = aa_of_digits(table, 3 - d2, 3 - d1, 3 - d0);
    const uint64_t arc1 = (uint64_t)ar * kC1, h2f = hp.seed ^ mix_k2((uint64_t)af) ^ (uint64_t)W;
    ctab[tid0] = arc1; ctab[64 + tid0] = h2f; ctab[128 + tid0] = af | (ar << 8);
  }
  if (W == 9) for (int e = tid0; e < 256; e += THREADS) k2tab[e] = hp.seed ^ mix_k2((uint64_t)e) ^ (uint64_t)W;
  if (tid0 == 0) st_ctl[0] = 0;

  const uint32_t thr_hi1 = open_thr<true>(hp.thr);
  W2 seedw{(uint32_t)hp.seed ^ (uint32_t)W, (uint32_t)(hp.seed >> 32)};   // in vector registers: see k_dna_rolling (sketch_dna_kernels.hip)
  asm volatile("" : "+v"(seedw.lo), "+v"(seedw.hi));
  const uint64_t ntiles = (b.len + TILE - 1) / TILE;
  const uintptr_t gend = ((uintptr_t)(b.seq + b.len) + 15) & ~(uintptr_t)15;
  const uint32_t nsteps = ((R + (uint32_t)KB - 1 + 11) / 12) * 12;   // bases walked per lane: whole triples of dwords
  const uint32_t warm_end = ((uint32_t)(KB - 1) / 12) * 12;          // iterations [0, warm_end) end before any window is complete
  // the end of the valid part of record r: a record shorter than ksize adds nothing (src/lib.rs:257)
  auto valid_end = [&](uint32_t r) -> uint64_t {
    const uint64_t s0 = b.starts[r], s1 = b.starts[r + 1];
    return s1 - s0 >= hp.ksize ? s1 : s0;
  };

  for (uint64_t tix = blockIdx.x; tix < ntiles; tix += gridDim.x) {
    // The lane number, re-read per tile behind an opaque asm: the compiler otherwise computes tid << logR and friends
    // once, ahead of this loop, and -- the main loop holding every register -- spills them; their reload at every tile
    // came from memory (the streamed input evicts the scratch lines from the L2 in between): 11 % more bytes fetched
    // than the input holds, 26 % for W = 10 (TCC_EA0_RDREQ, profiles/r02_ea_read_requests.txt).
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const uint64_t T0 = tix * TILE;
    const uintptr_t g0 = (uintptr_t)(b.seq + T0);
    const uintptr_t ga = g0 & ~(uintptr_t)15;
    const uint32_t m = (uint32_t)(g0 - ga);
    const uint32_t nchunks = (m + (uint32_t)TILE + (uint32_t)KB + 12 + 8 + 15) >> 4;
    __syncthreads();
    uint32_t high = 0;
    for (uint32_t c = tid; c < nchunks; c += THREADS) {
      uintptr_t addr = ga + ((uintptr_t)c << 4);
      uint4 v = make_uint4(0, 0, 0, 0);
      if (addr < gend) v = *reinterpret_cast<const uint4*>(addr);
      high |= v.x | v.y | v.z | v.w;
      uint32_t x = c << 4;
      uint32_t o = (x >> 2) + (x >> logR);
      tile[o] = v.x; tile[o + 1] = v.y; tile[o + 2] = v.z; tile[o + 3] = v.w;
    }
    if (high & 0x80808080u) atomicOr(high_flag, 1u);      // (bytes of the 16-byte granules around the batch may flag too: harmless)
    __syncthreads();

    const uint64_t p0 = T0 + ((uint64_t)tid << logR);     // my first window start position
    if (p0 < b.len) {
    const uint32_t nk = (b.len - p0) < R ? (uint32_t)(b.len - p0) : R;
    const uint32_t hi_ok = nk + (uint32_t)KB - 1;

    uint32_t rec = 0;
    uint64_t cur_end = b.vend0;
    if (multi) rec = find_record_in_tile(b, hp.ksize, tix, p0, &cur_end);
    uint32_t lim = 0;
    if (cur_end > p0) lim = (cur_end - p0) > 0xfffffffeull ? 0xffffffffu : (uint32_t)(cur_end - p0);
    uint32_t vstart = 0;                                  // first base index after the last record start / dropped base
    uint32_t rstart = 0;                                  // first base index of the record the walk is in
    uint32_t g_lo = 0, g_span = 0;
    auto set_clean_window = [&](bool warm) {
      const uint32_t lim2 = warm ? lim : (lim < hi_ok ? lim : hi_ok);
      g_lo = warm ? vstart : vstart + (uint32_t)KB - 1;
      g_span = lim2 >= g_lo + 4 ? lim2 - 3 - g_lo : 0u;
    };

    const uint32_t xu = m & ~3u;
    uint32_t ta = xu + ((uint32_t)tid << logR);
    ta = ta + ((ta >> logR) << 2);
    const uint32_t sh = m & 3u;
    uint32_t cur = tile[ta >> 2];
    ta += ((xu + 4u) & (R - 1)) == 0 ? 8u : 4u;
    uint32_t nxt = tile[ta >> 2];                         // always one dword ahead: its latency hides behind the hashing
    uint32_t pcode = 0;                                   // digits of the previous group, one per byte
    // per reading frame (base index mod 3): the forward and the reverse-complement residue strings (for W == 9 the
    // top dword of Sf is the last table entry as it came -- only its low byte is ever used -- and Sr keeps k1's 8 bytes)
    uint32_t Sf[3][ND], Sr[3][ND];
    uint64_t Mr[3];                                       // W >= 8: (first 8 residues of the reverse-complement string) * c1
#pragma unroll
    for (int t = 0; t < 3; t++) {
      Mr[t] = 0;
#pragma unroll
      for (int d = 0; d < ND; d++) { Sf[t][d] = 0; Sr[t][d] = 0; }
    }

    // four bases (one dword of the tile); PH = (base index / 4) mod 3 fixes which frame each base completes
    auto group = [&](uint32_t i0, auto phase, auto hashing) {
      constexpr int PH = decltype(phase)::value;
      constexpr bool kHash = decltype(hashing)::value;
      // W == 9, reverse strand: k2 is the residue that leaves k1 -- byte 7 of the string as it stands before the base
      // (for the group's fourth base, which shares its frame with the first: byte 6 of the string before the group).
      // Nothing of this group is needed for it, so the four look-ups go first and overlap with everything below.
      uint64_t h2r[4] = {0, 0, 0, 0};
      if (kHash && W == 9) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint32_t s1 = Sr[(4 * PH + q) % 3][1];
          h2r[q] = *reinterpret_cast<const uint64_t*>(reinterpret_cast<const char*>(k2tab) + (q < 3 ? byte_shl<3, 3>(s1) : byte_shl<3, 2>(s1)));
        }
      }
      const uint32_t d = __builtin_amdgcn_alignbyte(nxt, cur, sh);
      cur = nxt;
      const uint32_t xn = xu + i0 + 8;
      ta += (xn & (R - 1)) == 0 ? 8u : 4u;
      nxt = tile[ta >> 2];                                 // for the next group
      const uint32_t u4 = d & 0xDFDFDFDFu;
      const uint32_t c2 = (u4 >> 1) & 0x03030303u;
      const uint32_t code4 = c2 ^ ((c2 >> 1) & 0x01010101u);
      const uint32_t exp4 = __builtin_amdgcn_perm(0u, 0x54474341u, code4);
      const uint32_t diff4 = u4 ^ exp4;
      uint32_t okmask = 0xFu, slowmask = 0;
      if (!(diff4 == 0 && i0 - g_lo < g_span)) {
        okmask = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint32_t i = i0 + q;
          uint32_t bad = (diff4 >> (8 * q)) & 0xffu;
          if (i >= lim) {
            const uint64_t qpos = p0 + i;
            if (multi) {
              while (rec + 1 < b.nrec && qpos >= b.starts[rec + 1]) { rec++; vstart = i; rstart = i; }
              cur_end = valid_end(rec);
            }
            if (qpos >= cur_end) { bad = 1; lim = i + 1; }
            else lim = (cur_end - p0) > 0xfffffffeull ? 0xffffffffu : (uint32_t)(cur_end - p0);
          }
          if (bad) vstart = i + 1;
          if (kHash) {
            const bool inrun = i + 1 >= (uint32_t)KB && i < hi_ok;
            const bool simple = inrun && (i + 1 >= vstart + (uint32_t)KB);
            okmask |= simple ? (1u << q) : 0u;
            // A span that is not clean goes to the codon-by-codon walk -- unless it STARTS in an earlier record than
            // this base: its record then ends before 3W bases are through, and no window starts there.  (Every record
            // boundary makes 3W - 1 such spans; sending them through the walk cost a tenth of the kernel's time at
            // one boundary per 1 MB.)
            slowmask |= (inrun && !simple && i + 1 >= rstart + (uint32_t)KB) ? (1u << q) : 0u;
          }
        }
        set_clean_window(!kHash);
      }
      // Codon numbers of the codons that END at the group's four bases.  e4 = digits of bases i0-2 .. i0+1, one per
      // byte; x | x >> 6 | x >> 12 gathers three consecutive bytes' digits into the first one's byte (oldest lowest).
      const uint32_t e4 = __builtin_amdgcn_alignbyte(code4, pcode, 2);
      pcode = code4;
      const uint32_t ix01 = e4 | (e4 >> 6) | (e4 >> 12);              // bytes 0, 1: bases 0, 1
      const uint32_t ix23 = code4 | (code4 >> 6) | (code4 >> 12);     // bytes 0, 1: bases 2, 3
      // the four look-ups are issued together, ahead of the hashing they feed
      uint32_t eaa[4];
      uint64_t et1[4], h2f[4] = {0, 0, 0, 0};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t off = (q & 1) ? byte_shl<3, 1>(q < 2 ? ix01 : ix23) : byte_shl<3, 0>(q < 2 ? ix01 : ix23);
        const char* at = reinterpret_cast<const char*>(ctab) + off;
        if (W >= 8) et1[q] = *reinterpret_cast<const uint64_t*>(at);
        if (kHash && W == 9) h2f[q] = *reinterpret_cast<const uint64_t*>(at + 512);
        eaa[q] = *reinterpret_cast<const uint32_t*>(at + 1024);
      }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int t = (4 * PH + q) % 3;                    // reading frame completed by this base (lane-relative)
        const uint32_t e = eaa[q];                         // residue | residue of the reverse complement << 8
        // forward string: drop the oldest residue (byte 0), the new one becomes byte W-1
#pragma unroll
        for (int dd = 0; dd < ND - 1; dd++) Sf[t][dd] = __builtin_amdgcn_alignbyte(Sf[t][dd + 1], Sf[t][dd], 1);
        if (W == 9) Sf[t][ND - 1] = e;
        else Sf[t][ND - 1] = __builtin_amdgcn_perm(e, Sf[t][ND - 1], ((W - 1) & 3) == 0 ? 0x0c0c0c04u : ((W - 1) & 3) == 1 ? 0x0c0c0401u : ((W - 1) & 3) == 2 ? 0x0c040201u : 0x04030201u);
        // reverse-complement string: the new residue is its FIRST (byte 0), the oldest (byte W-1) falls off.
        // W >= 8: k1 * c1 rolls -- k1' = k1 << 8 | new (mod 2^64), and a left shift commutes with the multiplication:
        // (k1 * c1)' = (k1 * c1) << 8 + new * c1 (table), two instructions instead of a 64 x 64 multiply.
#pragma unroll
        for (int dd = ND - 1; dd > 0; dd--) {
          if (W == 9 && dd == 2) continue;
          const bool last = dd == ND - 1 && (W & 3) != 0;   // partial top dword: keep the bytes past W zero
          Sr[t][dd] = !last ? __builtin_amdgcn_alignbyte(Sr[t][dd], Sr[t][dd - 1], 3)
                            : __builtin_amdgcn_perm(Sr[t][dd], Sr[t][dd - 1], (W & 3) == 1 ? 0x0c0c0c03u : (W & 3) == 2 ? 0x0c0c0403u : 0x0c050403u);
        }
        Sr[t][0] = __builtin_amdgcn_perm(e, Sr[t][0], 0x02010005u);
        if (W >= 8) {
          uint64_t m16;
          asm("v_lshl_add_u64 %0, %1, 4, 0" : "=v"(m16) : "v"(Mr[t]));
          asm("v_lshl_add_u64 %0, %1, 4, %2" : "=v"(Mr[t]) : "v"(m16), "v"(et1[q]));
        }
        if (kHash && i0 + q + 1 >= (uint32_t)KB && i0 + q < R + (uint32_t)KB - 1) {   // uniform: a window of some lane's run can be complete here
          W2 fa, fb, ra, rb;
          const W2 k2f{ND > 2 ? Sf[t][ND > 2 ? 2 : 0] : 0u, ND > 3 ? Sf[t][ND > 3 ? 3 : 0] : 0u};
          const W2 k2r{ND > 2 ? Sr[t][ND > 2 ? 2 : 0] : 0u, ND > 3 ? Sr[t][ND > 3 ? 3 : 0] : 0u};
          murmur_short<W>(w2_mul(W2{Sf[t][0], Sf[t][1]}, kC1), k2f, seedw, h2f[q], fa, fb);
          murmur_short<W>(W >= 8 ? w2_split(Mr[t]) : w2_mul(W2{Sr[t][0], Sr[t][1]}, kC1), k2r, seedw, h2r[q], ra, rb);
          if (open_hi_sum1<true>(fa, fb) <= thr_hi1 || open_hi_sum1<true>(ra, rb) <= thr_hi1) {   // ~2 in `scaled` positions get here
            uint32_t om = okmask;
            asm volatile("" : "+v"(om));
            const uint64_t hf = open_full(fa, fb), hr = open_full(ra, rb);
            if ((om >> q) & 1u) {
              const uint64_t a = p0 + i0 + q + 1 - KB;      // first base of the span; see k_protein_positions
              if (hf <= hp.thr) stage_emit(stage, sink, hf, a << 1);
              if (hr <= hp.thr) stage_emit(stage, sink, hr, (a << 1) | 1u);
            }
          }
        }
      }
      if (kHash && slowmask) {
#pragma unroll 1
        for (int q = 0; q < 4; q++)
          if ((slowmask >> q) & 1u) {                     // for k_spliced_windows
            const uint32_t at = atomicAdd(slow_count, 1u);
            if (at < kSplicedCap) slow_list[at] = p0 + i0 + q + 1 - KB;
            else atomicOr(high_flag, 2u);
          }
      }
    };

    set_clean_window(true);
    uint32_t i0 = 0;
    for (; i0 < warm_end; i0 += 12) {
      group(i0, std::integral_constant<int, 0>{}, std::false_type{});
      group(i0 + 4, std::integral_constant<int, 1>{}, std::false_type{});
      group(i0 + 8, std::integral_constant<int, 2>{}, std::false_type{});
    }
    set_clean_window(false);
    for (; i0 < nsteps; i0 += 12) {
      group(i0, std::integral_constant<int, 0>{}, std::true_type{});
      group(i0 + 4, std::integral_constant<int, 1>{}, std::true_type{});
      group(i0 + 8, std::integral_constant<int, 2>{}, std::true_type{});
    }
    }  // p0 < b.len

    stage_flush(stage, sink, tid, THREADS);
  }
}

// protein arm, phase 2: a window starts at every kept residue and takes the next `win` kept
// residues of the same segment (dropped codons are spliced out, quirk Q8).
__device__ __forceinline__ void hash_window_slow(const uint8_t* __restrict__ res, uint64_t g, uint64_t end, uint32_t win,
                                                 const HashParams& hp, uint64_t thr, const CandSink& sink,
                                                 const Stage& stage) {
  if (res[g] == kDropped) return;
  Mm3Stream st(hp.seed);
  uint32_t got = 0;
  for (uint64_t q = g; q < end && got < win; q++) {
    uint32_t c = res[q];
    if (c != kDropped) { st.push(c); got++; }
  }
  if (got < win) return;
  uint64_t h = st.finish();
  if (h <= thr) stage_emit(stage, sink, h, hp.pos_base + g);
}

constexpr int kWinRun = 8;
// W: compile-time window length (0 = run-time `win_rt`): with W known the loads, the byte shifts and
// murmur's block / tail structure are all static
template <int W>
__device__ __forceinline__ void hash_run(const uint8_t* __restrict__ res, const uint64_t* __restrict__ seg_off,
                                         uint32_t nseg, uint32_t win_rt, const HashParams& hp, uint64_t thr,
                                         const CandSink& sink, const Stage& stage, bool aligned, uint64_t g0,
                                         uint64_t blk_seg_end, const uint64_t* k2lut) {
  {
    const uint32_t win = W ? (uint32_t)W : win_rt;
    // the workgroup's first segment was looked up once with uniform (scalar) loads; only lanes
    // past its end search for their own
    uint64_t end = blk_seg_end;
    if (g0 >= end) end = seg_off[find_record(seg_off, nseg, g0) + 1];
    const uint64_t last = g0 + kWinRun < hp.range_hi ? g0 + kWinRun : hp.range_hi;  // window starts [g0, last)
    bool fast = aligned && last == g0 + kWinRun && g0 + kWinRun - 1 + win <= end;
    uint32_t D[12];  // 48 bytes: 8 starts + up to 32-byte windows, little-endian dwords
    if (fast) {
      const uint2* src = reinterpret_cast<const uint2*>(res + g0);
      const int nw = (kWinRun + (int)win - 1 + 7) >> 3;  // 8-byte words covering the stretch
      uint32_t anydrop = 0;
#pragma unroll
      for (int i = 0; i < 6; i++) {
        uint2 v = make_uint2(0, 0);
        if (i < nw) v = src[i];
        D[2 * i] = v.x; D[2 * i + 1] = v.y;
        if (i < nw) {
          // a byte equal to 0xFF anywhere in the loaded words (bytes past the stretch may flag too: harmless)
          uint32_t nx = ~v.x, ny = ~v.y;
          anydrop |= ((nx - 0x01010101u) & ~nx & 0x80808080u) | ((ny - 0x01010101u) & ~ny & 0x80808080u);
        }
      }
      if (anydrop) fast = false;
    }
    if (!fast) {
      for (uint64_t g = g0; g < last; g++) {
        uint64_t e = end;
        if (g >= end) e = seg_off[find_record(seg_off, nseg, g) + 1];
        hash_window_slow(res, g, e, win, hp, thr, sink, stage);
      }
      return;
    }
    const int nblocks = (int)win >> 4, tail = (int)win & 15;
#pragma unroll
    for (int j = 0; j < kWinRun; j++) {
      // window j = bytes [j, j+win) of the stretch
      uint32_t Wd[8];
#pragma unroll
      for (int d = 0; d < 8; d++) {
        const int lo = d + (j >> 2);
        Wd[d] = (4 * d < (int)win) ? __builtin_amdgcn_alignbyte(D[lo + 1 < 12 ? lo + 1 : 11], D[lo], j & 3) : 0u;
        const int nb = (int)win - 4 * d;
        if (nb > 0 && nb < 4) Wd[d] &= (1u << (8 * nb)) - 1u;
      }
      uint64_t h1 = hp.seed, h2 = hp.seed;
#pragma unroll
      for (int blk = 0; blk < 2; blk++) {
        const uint64_t k1 = Wd[4 * blk] | ((uint64_t)Wd[4 * blk + 1] << 32);
        const uint64_t k2 = Wd[4 * blk + 2] | ((uint64_t)Wd[4 * blk + 3] << 32);
        if (blk < nblocks) mm3_block(h1, h2, k1, k2);
        else if (blk == nblocks) {
          // nine residues: k2 is a single byte, its mix comes from a 256-entry table (2 of the 8
          // 64-bit multiplies of the hash)
          if (W == 9) h2 ^= k2lut[k2 & 0xffu];
          else if (tail > 8) h2 ^= mix_k2(k2);
          if (tail > 0) h1 ^= mix_k1(k1);
        }
      }
      const uint64_t h = mm3_finish(h1, h2, (uint64_t)win);
      if (h <= thr) stage_emit(stage, sink, h, hp.pos_base + g0 + j);
    }
  }
}

// One lane owns 8 consecutive window starts and reads the 8+win-1 residues they cover once
// (aligned 8-byte loads).  When that stretch lies inside one segment and holds no dropped codon --
// the normal case -- every window is a byte-shifted view of those registers; otherwise the lane
// falls back to the residue-by-residue walk.  win <= 32 for the fast path.
template <int W>
__global__ __launch_bounds__(256) void k_hash_windows(const uint8_t* __restrict__ res,
                                                      const uint64_t* __restrict__ seg_off,
                                                      uint32_t nseg, uint32_t win, HashParams hp,
                                                      CandSink sink, uint32_t stage_cap) {
  extern __shared__ __attribute__((aligned(16))) uint32_t wsm[];
  __shared__ uint64_t k2lut[W == 9 ? 256 : 1];
  const Stage stage{wsm, reinterpret_cast<uint64_t*>(wsm + 4), reinterpret_cast<uint64_t*>(wsm + 4) + stage_cap, stage_cap};
  if (threadIdx.x == 0) wsm[0] = 0;
  if (W == 9) k2lut[threadIdx.x] = mix_k2((uint64_t)threadIdx.x);   // 256 threads, 256 byte values
  __syncthreads();
  const uint64_t thr = hp.thr;
  const bool aligned = ((hp.range_lo | (uintptr_t)res) & 7) == 0 && win <= 32 && win >= 1;
  // a workgroup owns a contiguous run of passes (2048 window starts each): the segment of the
  // pass start is searched once and then walked forward with uniform loads
  const uint64_t pass = (uint64_t)blockDim.x * kWinRun;
  const uint64_t npass = (hp.range_hi - hp.range_lo + pass - 1) / pass;
  const uint64_t per_wg = (npass + gridDim.x - 1) / gridDim.x;
  const uint64_t p_begin = (uint64_t)blockIdx.x * per_wg;
  const uint64_t p_end = p_begin + per_wg < npass ? p_begin + per_wg : npass;
  uint32_t seg = 0;
  if (p_begin < p_end) seg = find_record(seg_off, nseg, hp.range_lo + p_begin * pass);
  // the loop bound is the same for every lane of the workgroup: the flush inside synchronises
  for (uint64_t ps = p_begin; ps < p_end; ps++) {
    const uint64_t b0 = hp.range_lo + ps * pass;
    const uint64_t g0 = b0 + (uint64_t)threadIdx.x * kWinRun;
    while (seg + 1 < nseg && b0 >= seg_off[seg + 1]) seg++;   // b0 is uniform
    const uint64_t blk_seg_end = seg_off[seg + 1];
    if (g0 < hp.range_hi) hash_run<W>(res, seg_off, nseg, win, hp, thr, sink, stage, aligned, g0, blk_seg_end, k2lut);
    // a pass covers only 2048 windows: flushing (a returning global atomic) every pass would cost
    // more than the hashing; wait until the stage is half full
    stage_flush(stage, sink, threadIdx.x, blockDim.x, stage_cap / 2);
  }
  stage_flush(stage, sink, threadIdx.x, blockDim.x);
}

}  // namespace

// ---------------------------------------------------------------------------------
// launchers

void launch_translate(const SeqBatch& b, const uint64_t* seg_off, uint32_t nseg, uint64_t total, uint32_t ksize, uint32_t alphabet,
                      uint8_t* residues, uint32_t* bad_utf8, hipStream_t s) {
  if (total == 0) return;
  hipLaunchKernelGGL(k_translate, dim3(sketch_grid(b.len, kTrTile, 16384)), dim3(kTrThreads), 0, s, b, seg_off, nseg, ksize, alphabet,
                     residues, bad_utf8);
  HIP_CHECK(hipGetLastError());
}

bool launch_protein_fused(const SeqBatch& b_in, const uint64_t* seg_offsets, uint32_t win, const HashParams& p,
                          const CandSink& sink, uint32_t* high_flag, Device& dev, hipStream_t s) {
  if (b_in.len == 0) return true;
  if (!(win == 7 || win == 9 || win == 10)) return false;     // the usual protein k-mer sizes (ksize 21 / 27 / 30)
  int logR = SMH_PF_LOGR;
  while (logR > 5 && (b_in.len >> logR) < (uint64_t)dev.cu_count() * 512 * 2) logR--;
  const uint64_t tile = 512ull << logR;
  const uint64_t ntiles = (b_in.len + tile - 1) / tile;
  const int grid = (int)(ntiles < (uint64_t)dev.cu_count() * 8 ? ntiles : (uint64_t)dev.cu_count() * 8);
  const uint32_t x_bytes = (uint32_t)tile + 3 * win + 12 + 96;
  // two windows per position pass with probability (thr + 1) / 2^64 each
  long double expect = 2.0L * (long double)tile * (((long double)p.thr + 1.0L) / 18446744073709551616.0L);
  uint32_t stage_cap = expect * 2.0L + 64.0L > 2048.0L ? 2048u : (uint32_t)(expect * 2.0L + 64.0L);
  if (stage_cap < 128) stage_cap = 128;
  const size_t lds = 16 + (size_t)stage_cap * 8 * (sink.pos ? 2 : 1) + x_bytes + 4 * ((x_bytes >> logR) + 2);
  const SeqBatch b = with_tile_records(b_in, p.ksize, 0, tile, ntiles, dev, s);
  // the list of span starts for k_spliced_windows: [count][starts], in the shared scratch (used up before this returns'
  // successors on the stream -- the fold's sort -- claim it)
  dev.scratch.ensure(16 + (size_t)kSplicedCap * 8);
  uint32_t* slow_count = dev.scratch.as<uint32_t>();
  uint64_t* slow_list = reinterpret_cast<uint64_t*>(dev.scratch.as<char>() + 16);
  HIP_CHECK(hipMemsetAsync(slow_count, 0, 4, s));
#define SMH_PF(W_) hipLaunchKernelGGL((k_protein_fused<W_, 512>), dim3(grid), dim3(512), lds, s, b, p, sink, logR, stage_cap, high_flag, \
                                      slow_list, slow_count)
  if (win == 7) SMH_PF(7); else if (win == 9) SMH_PF(9); else SMH_PF(10);
#undef SMH_PF
  hipLaunchKernelGGL(k_spliced_windows, dim3(64), dim3(256), 0, s, b, p, sink, win, slow_list, slow_count);
  if (sink.pos)   // (a << 1 | strand) -> residue index of the six-frame layout
    hipLaunchKernelGGL(k_protein_positions, dim3(dev.cu_count() * 4), dim3(256), 0, s, sink.pos, sink.count, sink.capacity, b.starts,
                       b.nrec, b.len, seg_offsets, 3 * win, p.pos_base);
  HIP_CHECK(hipGetLastError());
  return true;
}

void launch_hash_windows(const uint8_t* bytes, uint64_t total, const uint64_t* seg_offsets,
                         uint32_t nseg, uint32_t win, const HashParams& p, const CandSink& sink,
                         hipStream_t s) {
  (void)total;
  if (p.range_hi <= p.range_lo) return;
  const uint32_t stage_cap = 1024;
  const size_t lds = 16 + (size_t)stage_cap * 8 * (sink.pos ? 2 : 1);
  const dim3 grid(sketch_grid((p.range_hi - p.range_lo + kWinRun - 1) / kWinRun, 256, 16384));
#define SMH_HW(W_) hipLaunchKernelGGL(k_hash_windows<W_>, grid, dim3(256), lds, s, bytes, seg_offsets, nseg, win, p, sink, stage_cap)
  // the usual protein k-mer sizes (ksize 21 / 27 / 30 nucleotides) get static instantiations
  if (win == 7) SMH_HW(7); else if (win == 9) SMH_HW(9); else if (win == 10) SMH_HW(10); else SMH_HW(0);
#undef SMH_HW
  HIP_CHECK(hipGetLastError());
}

}  // namespace smh
