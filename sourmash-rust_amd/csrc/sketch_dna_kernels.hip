// sketch_dna_kernels.hip -- gfx950 kernels for the DNA arm of KmerMinHash::add_sequence
// (reference src/lib.rs:252-274) and its validation:
//
//   k_dna_rolling<K>   DNA arm, ksize <= 128 (2, 4 or 8 32-bit limbs per packed window).  One lane owns a run of R
//                      consecutive k-mer start positions; the tile is read from HBM once with coalesced
//                      16-byte loads and staged in LDS; each lane rolls two 2-bit packed windows (the forward
//                      k-mer, first base least significant, and its complement, first base most significant
//                      = the reverse complement, first base least significant), picks the canonical strand
//                      with one 64-bit compare, takes the first multiply of every murmur word from LDS
//                      product tables indexed by the 2-bit digits (the ASCII bytes are never formed) and
//                      runs the rest of MurmurHash3 x64_128 (first word) on 32-bit halves in registers.
//                      replaces: src/lib.rs:260-267 (+ revcomp 677-689, _checkdna 795-804,
//                      _hash_murmur 33-35) and the `hash <= max_hash` filter of add_hash 198.
//   k_dna_generic      same contract for any ksize, one lane per k-mer, byte-wise.
//   k_first_invalid    first byte outside [ACGTacgt] per record (force=false, lib.rs:268-273); k_first_bad_record
//                      finds the first offending record on the device.
//   k_record_stats     counts the records of at least ksize bases and the protein arm's positions for batches of many
//                      records (lib.rs:257).
//
// MurmurHash3, the 32-bit halves (W2) and the open digest are murmur_device.hpp's; the LDS stage and the record look-ups
// sketch_device.hpp's; the per-tile record table comes from with_tile_records (sketch_launch.hpp, sketch_kernels.hip).
// All arithmetic is 64-bit integer; results are bit-exact with the reference by construction
// and checked against oracle/ in tests/.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "device.hpp"
#include "kernels.hpp"
#include "murmur_device.hpp"
#include "sketch_device.hpp"
#include "sketch_launch.hpp"

namespace smh {
namespace {

// ---------------------------------------------------------------------------------
// DNA arm, rolling 2-bit windows, ksize <= 128
// Product tables.  A k-mer reaches murmur as 8-byte words of ASCII letters, and the first thing
// murmur does with a word is multiply it by c1 (k1 words) or c2 (k2 words).  Multiplication
// distributes over the word's two 4-letter halves,  w*c = lo*c + ((hi*c) << 32)  (mod 2^64), and a
// half is one of 256 strings, so the products come from tables indexed by the 2-bit digits the
// kernel already holds: P1[i] = ascii4(i)*c1, P2[i] = ascii4(i)*c2 as u64 (the high half of a word
// needs only the low dword of the entry), plus one small table for the k-mer's last, partial group
// of letters.  This replaces the digit -> ASCII table AND a third of the 64-bit multiplies.
// One copy of the tables per workgroup: replicas (per lane parity ... per 16 lanes) were measured
// and never paid (1, 2: 37.8 ms; 4, 8: 39.7; 16: 50.5 per 10 GB) -- with one copy the entry address
// is (digits << 3) plus an immediate, two full-rate instructions per group.
//
// Folded tables (packed tile).  Of a word's product M = W*c, the low dword m = a.lo comes from the low half's entry a
// alone, and the high dword is S = a.hi + B (B: the low dword of the high half's entry).  The rest of murmur's word mix
// is linear in S once m is fixed, so the part that depends on m alone is precomputed per entry:
//   k2 words (x c2, rotl 33, x c1):  rotl(M, 33) = 2S + T'(m), T'(m) = (m >> 31) | (m mod 2^31) << 33,
//                                    mixed = S * (2 c1) + T2(m),  T2 = T'(m) * c1
//   k1 words (x c1, rotl 31, x c2):  rotl(M, 31) = (S >> 1) + m * 2^31 + (S & 1) * 2^63, and c2 is odd:
//                                    mixed = (S >> 1) * c2 + T1(m) + (S << 63),  T1 = m * 2^31 * c2
// (all mod 2^64).  A low-half entry is {T, a.hi, 0} in 16 bytes, one ds_read_b128; the high halves read the packed low
// dwords as before.  The mix of a word is then one v_mad_u64_u32, one v_mul_lo_u32 and one add (k1: plus a shift and
// the top bit), instead of a 64-bit rotate (two v_alignbit), three v_mad_u64_u32 and an add.  The byte tile keeps the
// plain product tables: its 64 KiB tile leaves no room for two workgroups per CU with the larger ones.
constexpr int kLutEntries = 256 + 256 + 64 + 1;              // P1, P2, partial group, one zero entry (groups past the k-mer)
constexpr int kLutDwords = kLutEntries * 3;                  // u64 entries (4.5 KiB), then their low dwords once more, packed
// The high dword's cross term of a k2 word comes from the tables too.  With ch = hi32(2 c1), S * (2 c1) =
// S * lo32(2 c1) + ((S * ch mod 2^32) << 32), and mod 2^32 the product S * ch is linear in a.hi and B -- the wrap of
// a.hi + B drops out (2^32 * ch == 0) -- so a.hi * ch is added to the high dword of the low half's T2 (T2'') and the high
// halves of the k2 words read 8-byte entries {B, B' = B * ch}: mixed = S * lo32(2 c1) + T2'' + (B' << 32), one
// v_mad_u64_u32 and one add, no v_mul_lo_u32.  The k1 words' multiplier sees S >> 1, which is not linear in a.hi and B:
// their high halves stay on the packed dwords.
constexpr int kLutHiEntries = 256 + 64 + 1;                  // a high half's table: full groups, partial group, the zero entry
constexpr int kLutFoldB8 = kLutEntries * 4;                  // dword index of the k2 high halves' {B, B'} (8-byte aligned)
constexpr int kLutFoldB4 = kLutFoldB8 + kLutHiEntries * 2;   // dword index of the k1 high halves' packed low dwords
constexpr int kLutDwordsCross = kLutFoldB4 + kLutHiEntries;  // folded: 16-byte entries (9 KiB), {B, B'} (2.5 KiB), packed B (1.25 KiB)
constexpr int kLutDwordsFold = kLutEntries * 5;              // folded, cross term multiplied: 16-byte entries, then the packed low dwords
constexpr uint64_t kC1x2 = kC1 * 2;                          // (mod 2^64)

// The rest of a word's mix from a folded entry (see kLutDwordsFold): T = T1 or T2 of the low half, S = a.hi + B.
__device__ __forceinline__ W2 mix_k1_fold(uint32_t S, W2 T) {   // (S >> 1) * c2 + T1 + (S << 63)
  const uint32_t cl = (uint32_t)kC2, ch = (uint32_t)(kC2 >> 32), s1 = S >> 1;
  uint64_t p, cy;
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(p), "=s"(cy) : "v"(s1), "s"(cl), "v"(((uint64_t)T.hi << 32) | T.lo));
  uint32_t hi, top;
  asm("v_add_u32 %0, %1, %2" : "=v"(hi) : "v"((uint32_t)(p >> 32)), "v"(s1 * ch));
  asm("v_lshl_add_u32 %0, %1, 31, %2" : "=v"(top) : "v"(S), "v"(hi));
  return {(uint32_t)p, top};
}
// CROSS: S * lo32(2 c1) + T2'' + (B' << 32); otherwise S * (2 c1) + T2
template <bool CROSS>
__device__ __forceinline__ W2 mix_k2_fold(uint32_t S, W2 T, uint32_t Bp) {
  const uint32_t cl = (uint32_t)kC1x2, ch = (uint32_t)(kC1x2 >> 32);
  uint64_t p, cy;
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(p), "=s"(cy) : "v"(S), "s"(cl), "v"(((uint64_t)T.hi << 32) | T.lo));
  uint32_t hi;
  asm("v_add_u32 %0, %1, %2" : "=v"(hi) : "v"((uint32_t)(p >> 32)), "v"(CROSS ? Bp : S * ch));
  return {(uint32_t)p, hi};
}
// mix of word w (even: k1, odd: k2).  FOLD: M[w] = T of the low half's entry, S[w] = the word product's high dword and
// (CROSS, k2 words) P[w] = B' of the high half's entry; otherwise M[w] = word_w * (w even ? c1 : c2) and S, P are not used
template <bool FOLD, bool CROSS>
__device__ __forceinline__ W2 mix_word(int w, W2 M, uint32_t S, uint32_t P) {
  if (FOLD) return (w & 1) ? mix_k2_fold<CROSS>(S, M, P) : mix_k1_fold(S, M);
  return (w & 1) ? w2_mul(w2_rotl(M, 33), kC1) : w2_mul(w2_rotl(M, 31), kC2);
}
// h ^ m with the length KX xored into the low dword as well: a ^ b ^ c is v_bitop3_b32 with the truth table 0x96 (gfx950
// has no v_xor3_b32), and with the third operand an inline constant it issues at the rate of a plain v_xor_b32 (105
// lanes/clk/CU against 68 with three registers: tools/instr_rate.hip), so the xor of the length costs nothing
template <int KX>
__device__ __forceinline__ W2 w2_xor_len(W2 h, W2 m) {
  uint32_t lo;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(lo) : "v"(h.lo), "v"(m.lo), "n"(KX));
  return {lo, h.hi ^ m.hi};
}
// murmur64 from the table look-ups of the k-mer's words (mix_word).
// The digest is left OPEN one multiply early: (ka, kb) with h = open_full(ka, kb), filtered by open_hi_sum1.
// S32: the seed is below 2^32 (the launcher has checked it).  seedv.hi is never read: h1 and h2 start with a high dword
// that is zero at compile time, so the first xor into each is one instruction on the low dword (k1.hi and k2.hi pass
// through).  The folded constant seed * 5 + c stays the run-time 64-bit value.
// KX > 0: k at compile time and not a multiple of 16 (the kernels with S32 and a compile-time k): `^= len` rides on the
// tail words' xors (w2_xor_len); h2 has no tail word for k mod 16 <= 8 and keeps its own xor.
template <int L, bool FOLD, bool CROSS, bool S32 = false, int KX = 0>
__device__ __forceinline__ void murmur_kmer_pre(const W2 (&M)[2 * L], const uint32_t (&S)[2 * L], const uint32_t (&P)[2 * L], int K, uint64_t seed, W2 seedv,
                                                W2& a, W2& b) {
  W2 h1 = seedv, h2 = seedv;                            // (seedv: the seed's halves in vector registers, see k_dna_rolling)
  if (S32) { h1.hi = 0u; h2.hi = 0u; }
  const int nblocks = K >> 4, tail = K & 15;
#pragma unroll
  for (int blk = 0; blk < L; blk++) {
    const int w1 = 2 * blk, w2 = 2 * blk + 1;
    if (blk < nblocks) {
      h1 = w2_xor(h1, mix_word<FOLD, CROSS>(w1, M[w1], S[w1], P[w1]));
      // (rotl(h1, 27) + h2) * 5 + c; in the first block h2 is still the seed: rotl * 5 + (seed * 5 + c)
      if (blk == 0) h1 = w2_mul5_add(w2_rotl(h1, 27), seed * 5 + 0x52dce729u);
      else h1 = w2_mul5_add(w2_add(w2_rotl(h1, 27), h2), 0x52dce729u);
      h2 = w2_xor(h2, mix_word<FOLD, CROSS>(w2, M[w2], S[w2], P[w2]));
      h2 = w2_mul5_add(w2_add_keep(w2_rotl(h2, 31), h1), 0x38495ab5u);
    } else if (blk == nblocks) {
      if (KX > 0) {
        if ((KX & 15) > 8) h2 = w2_xor_len<KX>(h2, mix_word<FOLD, CROSS>(w2, M[w2], S[w2], P[w2]));
        else h2.lo ^= (uint32_t)KX;
        h1 = w2_xor_len<KX>(h1, mix_word<FOLD, CROSS>(w1, M[w1], S[w1], P[w1]));
        continue;
      }
      if (tail > 8) h2 = w2_xor(h2, mix_word<FOLD, CROSS>(w2, M[w2], S[w2], P[w2]));
      if (tail > 0) h1 = w2_xor(h1, mix_word<FOLD, CROSS>(w1, M[w1], S[w1], P[w1]));
    }
  }
  if (KX == 0) { h1.lo ^= (uint32_t)K; h2.lo ^= (uint32_t)K; }          // ^= len (K <= 128)
  w2_cross_add(h1, h2);
  a = w2_fmix_pre(h1); b = w2_fmix_pre(h2);           // first word of the digest = open_full(a, b)
}

// KT > 0: ksize fixed at compile time; KT == 0: any ksize the limb count allows, at run time.
// L = 32-bit limbs of a packed window: 2 for ksize <= 32, 4 for ksize <= 64, 8 for ksize <= 128.
// THREADS lanes per workgroup share the product tables; HB = hashes computed together in one straight-line
// block (independent murmur chains the scheduler can interleave).
// PR: thresholds are looked up per record (hp.thr_rec; grouped bottom-num batches) instead of the
// launch-uniform hp.thr
//
// Bookkeeping.  A lane walks its bases four at a time (one dword of the tile).  A group of four is
// CLEAN when all four bases are ACGT, none lies outside the current record's valid part, and all four
// windows that end in it are complete and belong to the lane's run: then there is nothing to decide
// per base.  One unsigned compare tells (g_span), and only groups that are not clean -- the first
// and the last one of a run that is not whole (see kEdgeFree), the ones around a record boundary
// or a non-ACGT byte -- take the per-base path below, which produces a 4-bit mask of the windows
// that may be emitted.
//
// PK: the tile is staged PACKED -- two bits per base (the 2-bit code the rolling needs anyway: the upper-casing, the
// encoding and the validity check are done once, by the lane that stages the bytes, 16 at a time) plus one "dirty" bit per
// source dword that holds a byte other than ACGT.  A lane's run of 128 bases is 32 bytes of LDS instead of 128: a 512-lane
// workgroup needs ~28 KB instead of ~73 KB, so FOUR workgroups share a CU (8 waves per SIMD instead of 4: the kernel waits
// on its own dependent murmur chains in a third of its wave cycles), and the hot path reads one LDS dword per
// 16 bases and decodes nothing.  Dirty dwords end the lane's window of clean groups like a record boundary does; the group
// then re-reads its four bytes from global memory (rare) and takes the per-base path with the same conditions as ever.
constexpr int kDnaCtlDwords = 8;   // the LDS header of k_dna_rolling (32 bytes: the staged hashes behind it stay 16-byte aligned)
// S32: hp.seed < 2^32, known to the launcher (murmur_kmer_pre); with a compile-time k the length's xor is folded too
// (w2_xor_len).  Only the packed two-limb kernels with a launch-uniform threshold have the variant; a seed at or above
// 2^32 runs the kernel without it, which is the code of before.
template <int KT, int THREADS, int HB, int L, bool PR = false, bool PK = false, int MINW = (PK ? 8 : 4), bool S32 = false>
__global__ __launch_bounds__(THREADS, MINW) void k_dna_rolling(SeqBatch b, HashParams hp, CandSink sink,
                                                                     int logR, uint32_t stage_cap, uint32_t* tile_ctr) {
  // LDS: static: the product tables (6.8 KiB, folded 11.3 KiB, folded with the cross term 12.8 KiB; a compile-time address, so a table read is one
  // ds_read with the table's base as its immediate offset); dynamic: [staged candidates: count,
  // hashes, positions][sequence tile]
  // folded tables (kLutDwordsFold) for the packed tile and k <= 32.  The byte tile and the 4- and 8-limb windows keep the plain
  // ones: the byte tile has no LDS to spare, and at L = 4 the folded look-ups push the kernel over 80 registers (spills).
  constexpr bool FOLD = PK && L == 2;
  // the k2 words' cross term from the tables (kLutDwordsCross).  Not in the per-record kernels: held to 64 registers for
  // eight waves per SIMD, they already spill, and the second dword of the {B, B'} reads makes them spill more.
  constexpr bool CROSS = FOLD && !PR;
  // the filter on the sum ka + kb (open_hi_sum1<true>, open_thr<true>).  Not in the per-record kernels on the folded
  // tables with a compile-time k (k = 21, 31): held to 64 registers they spill 28 bytes per lane, and the sum's register
  // pair next to ka and kb makes that 32 -- also with the sum's cross terms formed by 32-bit multiplies, which need no
  // further pair.  They keep the filter on both products (open_hi_sum1<false>, open_thr<false>).
  constexpr bool SUMF = !(PR && FOLD && KT != 0);
  __shared__ __attribute__((aligned(16))) uint32_t lut[CROSS ? kLutDwordsCross : (FOLD ? kLutDwordsFold : kLutDwords)];
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint32_t* st_ctl = smem;                                    // [0] = count, [1] = dirty tile, [2..3] = flush base, [4] = next tile
  uint64_t* st_hash = reinterpret_cast<uint64_t*>(st_ctl + kDnaCtlDwords);
  uint64_t* st_pos = st_hash + stage_cap;
  uint32_t* tile = reinterpret_cast<uint32_t*>(st_pos + (sink.pos ? stage_cap : 0));
  const Stage stage{st_ctl, st_hash, st_pos, stage_cap};

  const int K = KT ? KT : (int)hp.ksize;
  const int tid = threadIdx.x;
  const uint32_t R = 1u << logR;
  const uint64_t TILE = (uint64_t)THREADS << logR;
  // 2K-bit mask, limb by limb
  uint32_t MASK[L];
#pragma unroll
  for (int i = 0; i < L; i++) {
    const int bits = 2 * K - 32 * i;
    MASK[i] = bits >= 32 ? 0xffffffffu : (bits <= 0 ? 0u : ((1u << bits) - 1u));
  }
  const int top_limb = (2 * K - 2) >> 5, top_sh = (2 * K - 2) & 31;
  const bool multi = b.starts != nullptr;

  // product tables (see kLutEntries): entry e at u64 index e.
  // digit d -> "ACGT"[d], first digit in the low byte; the partial group holds the k-mer's last
  // K mod 4 letters (its multiplier follows the parity of the word it belongs to)
  const int g_last = (K - 1) >> 2, nb_last = K - 4 * g_last;      // nb_last == 4: no partial group
  const uint64_t c_last = ((g_last >> 1) & 1) ? kC2 : kC1;
  uint64_t* ptab = reinterpret_cast<uint64_t*>(lut);
  for (int e = tid; e < kLutEntries; e += THREADS) {
    const uint32_t ent = (uint32_t)e;
    const uint32_t idx = ent & 255u;
    const int nb = ent < 512 ? 4 : (ent < 576 ? nb_last : 0);
    uint32_t v = 0;
    for (int j = 0; j < nb; j++) v |= ((0x54474341u >> (8 * ((idx >> (2 * j)) & 3))) & 0xffu) << (8 * j);
    const uint64_t c = ent < 256 ? kC1 : (ent < 512 ? kC2 : c_last);
    const uint64_t prod = (uint64_t)v * c;
    // The high half of a word needs only the product's low dword.  Read out of the 8-byte entries those look-ups
    // touch the even banks only; the packed copy spreads them over all 64 (SQ_LDS_BANK_CONFLICT 43 -> ... per 64 k-mers).
    if (FOLD) {
      // {T, a.hi, 0}: T1 for the k1 words' multiplier c1, T2'' for c2 (the zero entry stays zero: mix(0) = 0)
      const uint64_t mm = (uint32_t)prod;
      const uint32_t ahi = (uint32_t)(prod >> 32), ch = (uint32_t)(kC1x2 >> 32);
      const uint64_t t = c == kC1 ? (mm << 31) * kC2
                                  : ((mm >> 31) | ((mm & 0x7fffffffu) << 33)) * kC1 + (CROSS ? (uint64_t)(ahi * ch) << 32 : 0ull);
      reinterpret_cast<uint4*>(lut)[e] = make_uint4((uint32_t)t, (uint32_t)(t >> 32), ahi, 0u);
      // high halves: full groups of the k1 words -> packed B, of the k2 words -> {B, B'}; the partial group and the zero
      // entry go to both (a partial group is the high half of a k1 or of a k2 word, depending on k; when it is not that of
      // a k2 word its {B, B'} entries mean nothing and are never read)
      const uint32_t B = (uint32_t)prod;
      const uint32_t he = ent < 256 ? ent : ent - 256u;              // index in a high half's table
      if (!CROSS) lut[4 * kLutEntries + e] = B;
      else {
        if (ent < 256 || ent >= 512) lut[kLutFoldB4 + he] = B;
        if (ent >= 256) reinterpret_cast<uint2*>(lut + kLutFoldB8)[he] = make_uint2(B, B * ch);
      }
    } else {
      ptab[e] = prod;
      lut[2 * kLutEntries + e] = (uint32_t)prod;
    }
  }
  // table base (bytes) of every 4-letter group: a compile-time constant for a compile-time k, fixed for
  // the launch otherwise, so that the per-k-mer code is the same straight line either way
  uint32_t gbase[4 * L];
#pragma unroll
  for (int g = 0; g < 4 * L; g++) {
    const int nb = K - 4 * g;
    uint32_t ent0 = 576u;                                              // past the k-mer: the zero entry
    if (nb >= 4) ent0 = ((g >> 1) & 1) ? 256u : 0u;
    else if (nb > 0) ent0 = 512u;
    constexpr uint32_t esz = FOLD ? 16u : 8u;                          // bytes per low-half entry
    gbase[g] = (g & 1) ? esz * kLutEntries + ent0 * 4u : ent0 * esz;  // odd groups (high halves): the packed low dwords (CROSS: see below)
    if (CROSS && (g & 1)) {                                            // {B, B'} for a k2 word, packed B for a k1 word
      const uint32_t he = nb >= 4 ? 0u : (nb > 0 ? 256u : 320u);
      gbase[g] = (g & 2) ? 4u * kLutFoldB8 + he * 8u : 4u * kLutFoldB4 + he * 4u;
    }
  }
  if (tid == 0) st_ctl[0] = 0;

  const uint64_t span = hp.range_hi - hp.range_lo;
  const uint64_t ntiles = (span + TILE - 1) / TILE;
  const uintptr_t gend = ((uintptr_t)(b.seq + b.len) + 15) & ~(uintptr_t)15;
  const uint32_t nsteps = (R + (uint32_t)K - 1 + 3) & ~3u;  // bases walked per lane, multiple of 4
  const uint32_t warm_end = K > 4 ? ((uint32_t)(K - 1) & ~3u) : 0u;   // groups [0, warm_end) end before any window is complete

  // Tiles.  The launch has as many workgroups as are resident at once (resident_workgroups); a workgroup's first tile is
  // its own number.  tile_ctr == null (no more tiles than workgroups): that is all.  Otherwise the next tile is
  // gridDim.x + atomicAdd(tile_ctr, 1) -- the word is zero when the kernel starts -- so that whichever workgroup is done
  // first takes the next tile and the kernel's tail is one tile long, wherever the dispatcher placed the workgroups and
  // however slow single tiles (dirty dwords, record edges) or CUs are.  Lane 0 asks for it behind the staging barrier, so
  // that the round trip runs under the hashing loop, and leaves it in the LDS header; everybody reads it behind the first
  // barrier of stage_flush and lane 0 writes the word again only behind the next tile's staging barrier.  No workgroup
  // ever waits for another one.  (Not in the per-record kernels, which are never given a counter: held to 64 registers
  // they spill, and the second way round the loop made some of them spill more.)
  for (uint64_t tix = blockIdx.x; tix < ntiles;) {
    const uint64_t T0 = hp.range_lo + tix * TILE;
    const uint64_t thr = hp.thr;
    const uint32_t thr_hi1 = open_thr<SUMF>(hp.thr);
    // An operand in a scalar register halves the issue rate of a plain two-operand instruction (tools/instr_rate.hip):
    // what the hash xors in per k-mer lives in vector registers.
    W2 seedv{(uint32_t)hp.seed, S32 ? 0u : (uint32_t)(hp.seed >> 32)};
    if (S32) asm volatile("" : "+v"(seedv.lo));
    else asm volatile("" : "+v"(seedv.lo), "+v"(seedv.hi));
    uint64_t lthr = hp.thr;   // PR: threshold of the record the lane is in

    // ---- stage [T0, T0 + TILE + K - 1) in LDS: aligned 16-byte loads, one pad dword per R bytes
    const uintptr_t g0 = (uintptr_t)(b.seq + T0);
    const uintptr_t ga = g0 & ~(uintptr_t)15;
    const uint32_t m = (uint32_t)(g0 - ga);
    const uint32_t nchunks = (m + (uint32_t)TILE + 16 * L + 8 + 15 + (PK ? 32u : 0u)) >> 4;  // last lane reads < m+TILE+K+7 (PK: a dword ahead)
    const uint32_t nchunks_cap = (15u + (uint32_t)TILE + 16 * L + 8 + 15 + 32u) >> 4;     // (the same for the largest m: where the dirty bits start)
    __syncthreads();  // tables ready / previous tile fully consumed
    uint32_t* dirty = tile + (nchunks_cap + (nchunks_cap >> (logR - 4)) + 2);     // PK: one bit per source dword, behind the codes
    if (PK) {
      for (uint32_t c = tid; c < (nchunks >> 3) + 3; c += THREADS) dirty[c] = 0;
      if (tid == 0) st_ctl[1] = 0;                                   // "some dword of this tile is dirty"
      __syncthreads();
    }
    // chunks that lie inside the (16-byte padded) input: one 32-bit compare per chunk instead of a 64-bit address compare
    const uint64_t cin64 = gend > ga ? (uint64_t)(gend - ga) >> 4 : 0ull;
    const uint32_t cin = cin64 < nchunks ? (uint32_t)cin64 : nchunks;
    // "ACTG", the letters in the order of bits 1..2 of their codes, in a SCALAR register: v_perm_b32 is a three-operand form
    // at either rate, and a vector register held for the constant across the whole kernel costs the k-mer loop a spill
    uint32_t kActg;
    asm("s_mov_b32 %0, 0x47544341" : "=s"(kActg));
    for (uint32_t c = tid; c < nchunks; c += THREADS) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (c < cin) v = *reinterpret_cast<const uint4*>(ga + ((uintptr_t)c << 4));
      if (PK) {
        // 16 bases -> 32 bits of codes (base j of the chunk in bits 2j, 2j+1) + 4 dirty bits.  Per source dword: upper-case,
        // bits 1..2 of every letter (A0 C1 T2 G3, a Gray code of A0 C1 G2 T3), validity by re-expanding THAT code, and the
        // four 2-bit fields gathered into one byte by one v_dot4_u32_u8 with the weights 1, 4, 16, 64 (it issues a little
        // faster than v_mul_lo_u32 by 2^24 + 2^18 + 2^12 + 2^6: tools/instr_rate.hip).  The Gray code is turned into the
        // binary one once per 16 bases, on the assembled dword.  Every byte is encoded on its own: a valid base inside a
        // dirty dword keeps its correct code (the per-base path rolls the windows from it).
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
        uint32_t xany = 0, gray = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint32_t u4 = w4[q] & 0xDFDFDFDFu;
          const uint32_t g4 = (u4 >> 1) & 0x03030303u;
          xany |= u4 ^ __builtin_amdgcn_perm(0u, kActg, g4);
          gray |= __builtin_amdgcn_udot4(g4, 0x40100401u, 0u, false) << (8 * q);   // the dword's four codes in one byte
        }
        tile[c + (c >> (logR - 4))] = gray ^ ((gray >> 1) & 0x55555555u);   // one pad dword per run: lane-strided reads hit distinct banks
        if (xany) {
          // rare: some byte other than ACGT.  Which dwords hold one is found from the 16 bytes read again, so that the
          // common path carries one word of differences instead of four.
          const volatile uint32_t* src = reinterpret_cast<const volatile uint32_t*>(ga + ((uintptr_t)c << 4));
          uint32_t bad = 0;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const uint32_t u4 = (c < cin ? src[q] : 0u) & 0xDFDFDFDFu;
            bad |= u4 != __builtin_amdgcn_perm(0u, kActg, (u4 >> 1) & 0x03030303u) ? 1u << q : 0u;
          }
          atomicOr(&dirty[c >> 3], bad << (4u * (c & 7u)));
          st_ctl[1] = 1;
        }
      } else {
        uint32_t x = c << 4;
        uint32_t o = (x >> 2) + (x >> logR);
        tile[o] = v.x; tile[o + 1] = v.y; tile[o + 2] = v.z; tile[o + 3] = v.w;
      }
    }
    __syncthreads();
    if (!PR && tile_ctr && tid == 0) st_ctl[4] = atomicAdd(tile_ctr, 1u);   // the next tile (see above)

    const uint64_t p0 = T0 + ((uint64_t)tid << logR);  // my first k-mer start position
    if (p0 < hp.range_hi) {
    const uint32_t nk = (hp.range_hi - p0) < R ? (uint32_t)(hp.range_hi - p0) : R;
    const uint32_t hi_ok = nk + (uint32_t)K - 1;        // base index i ends a window of my run iff K-1 <= i < hi_ok

    // record bookkeeping: `lim` = index of the first base of my run that is not inside the
    // current record's valid part
    uint32_t rec = 0;
    uint64_t cur_end = b.vend0;
    if (multi) {
      rec = find_record_in_tile(b, 0, tix, p0, &cur_end);
      if (PR) lthr = hp.thr_rec[rec];
    }
    uint32_t lim = 0;
    if (cur_end > p0) lim = (cur_end - p0) > 0xfffffffeull ? 0xffffffffu : (uint32_t)(cur_end - p0);
    uint32_t vstart = 0;      // first base of the run of valid bases that reaches the current base
    // clean groups: g_lo <= i0 < g_lo + g_span  (see the kernel comment)
    uint32_t g_lo = 0, g_span = 0;
    // PK: bit g = group g of my run touches a source dword that holds a byte other than ACGT (dirty bits of the tile,
    // one per aligned dword of the input; a group whose bases straddle two dwords looks at both)
    uint64_t dmask = 0;
    if (PK && st_ctl[1]) {
      const uint32_t b0 = (m + ((uint32_t)tid << logR)) >> 2;
      const uint32_t* dw = reinterpret_cast<const uint32_t*>(tile) + (nchunks_cap + (nchunks_cap >> (logR - 4)) + 2);
      const uint32_t i = b0 >> 5, sft = b0 & 31u;
      const uint64_t lo64 = ((uint64_t)dw[i + 1] << 32) | dw[i];
      const uint32_t d2 = dw[i + 2];
      dmask = (lo64 >> sft) | (sft ? ((uint64_t)d2 << (64 - sft)) : 0ull);
      if (m & 3u) dmask |= (dmask >> 1) | ((uint64_t)((d2 >> sft) & 1u) << 63);
    }
    // The uniform guard of a hashing block, i0 + g0b + HB >= K && i0 + g0b < R + K - 1, hashes exactly the complete windows
    // of a full run when the blocks line up with base K - 1 ((K - 1) % HB == 0; R is a multiple of HB).  Then a run that has
    // seen no invalid base (vstart == 0) and that the range does not cut short (nk == R) needs no mask for its first and
    // its last hashing group either: its clean stretch starts with the group of base K - 1 and only `lim` and the dirty
    // bits end it -- the walk's last bases, past the run, must be valid for that, or the group goes base by base as before.
    constexpr bool kEdgeFree = KT > 0 && (KT - 1) % HB == 0;
    auto set_clean_window = [&](bool warm, uint32_t from_i) {
      const bool whole = warm || (kEdgeFree && vstart == 0 && nk == R);
      uint32_t lim2 = whole ? lim : (lim < hi_ok ? lim : hi_ok);
      if (PK) {
        const uint32_t g = from_i >> 2;
        const uint64_t rem = g < 64 ? (dmask >> g) : 0ull;
        if (rem) lim2 = min(lim2, (g + (uint32_t)__builtin_ctzll(rem)) * 4u);      // clean groups end before the next dirty one
      }
      g_lo = whole ? vstart : vstart + (uint32_t)K - 1;  // warm-up groups emit nothing: only validity matters
      g_span = lim2 >= g_lo + 4 ? lim2 - 3 - g_lo : 0u;
    };

    // tile address of the lane's current dword: one pad dword per R bytes; the running form adds 4
    // per group, and 4 more when the group crosses a multiple of R -- which it does for every lane
    // of the workgroup at once (lane runs start R apart), so the increment is a scalar
    const uint32_t xu = m & ~3u;                                     // uniform part of the lane's byte index
    uint32_t ta = xu + ((uint32_t)tid << logR);
    ta = ta + ((ta >> logR) << 2);                                   // byte offset in the padded tile
    const uint32_t sh = m & 3u;
    uint32_t cur = PK ? 0u : tile[ta >> 2];
    // PK: the codes of my run: chunk (16 bases, one dword) cq holds my base 16 * (cq - cq0) - (m & 15); w = the 16 bases of
    // the current quad of groups, aligned (base j of the quad in bits 2j), wc = their complements; both move down 8 bits per group
    uint32_t cq = (m >> 4) + ((uint32_t)tid << (logR - 4));
    const uint32_t sh2 = (m & 15u) * 2u;
    uint32_t pcur = PK ? tile[cq + (cq >> (logR - 4))] : 0u, w = 0, wc = 0;
    // two rolled windows of 2-bit digits in L limbs.  fle: the forward k-mer, first base least
    // significant.  cf: the COMPLEMENT of the forward k-mer, first base most significant -- which is
    // the reverse complement with ITS first base least significant.  Both candidates for the hashed
    // strand are therefore at hand as they are (first base low), and the reference's `kmer < rc`
    // (src/lib.rs:263; ASCII order A<C<G<T equals digit order) needs no complementing either: with
    // M = 4^k - 1, forward read first-base-most-significant is M - cf and the reverse complement read
    // that way is M - fle, so  kmer < rc  <=>  M - cf < M - fle  <=>  fle < cf.
    uint32_t cf[L], fle[L];
#pragma unroll
    for (int i = 0; i < L; i++) { cf[i] = 0; fle[i] = 0; }
    // k = 31, packed tile: the windows are not rolled base by base but taken once per base from state kept per GROUP,
    // with one funnel shift (v_alignbit) per limb.  fa = the forward window before the group, with the group's first
    // code in its spare top bits 62..63, so that {w >> 2, fa} is the forward stream and the window ending at base q of
    // the group is that stream >> 2(q+1).  cs = the complement window before the group; wr = the complements of the
    // quad's 16 codes in reverse order (base j of the quad in bits 30-2j), moved up 8 bits per group, so that the window
    // ending at base q is {cs, wr} << 2(q+1).  Per base: four v_alignbit and two masks, against two v_alignbit, two
    // v_and_or and five plain shifts/masks for rolling both windows one base at a time.
    constexpr bool kRoll31 = PK && L == 2 && KT == 31;
    // strand choice by a floating-point minimum: compile-time k <= 31 on the packed two-limb kernels (at k = 32, which the
    // run-time-k kernel serves, bit 63 can be set)
    constexpr bool kMinF64 = PK && L == 2 && KT > 0 && KT <= 31;
    uint32_t fa0 = 0, fa1 = 0, cs0 = 0, cs1 = 0, wr = 0;

    // one group of four bases; hashing = false for the warm-up groups
    auto group = [&](uint32_t i0, auto hashing) {
      constexpr bool kHash = decltype(hashing)::value;
      uint32_t code4 = 0, ccode4 = 0, diff4 = 0;
      if (PK) {
        if ((i0 & 12u) == 0) {                                       // uniform: a new dword of codes every 16 bases
          cq += 1;
          const uint32_t pnxt = tile[cq + (cq >> (logR - 4))];
          w = __builtin_amdgcn_alignbit(pnxt, pcur, sh2);
          pcur = pnxt;
          wc = ~w;
          if (kRoll31) {
            fa1 |= w << 30;                                          // (the last group of a quad left those bits zero)
            const uint32_t r = __builtin_bitreverse32(w);            // digits reversed, each digit's two bits swapped
            wr = ~(((r >> 1) & 0x55555555u) | ((r << 1) & 0xaaaaaaaau));
          }
        }
      } else {
        const uint32_t xn = xu + i0 + 4;                             // uniform: byte index of the next dword
        ta += (xn & (R - 1)) == 0 ? 8u : 4u;
        const uint32_t nxt = tile[ta >> 2];
        const uint32_t d = __builtin_amdgcn_alignbyte(nxt, cur, sh);
        cur = nxt;
        // four bases at once: upper-case, 2-bit code (A0 C1 G2 T3), validity by re-encoding
        const uint32_t u4 = d & 0xDFDFDFDFu;
        const uint32_t c2 = (u4 >> 1) & 0x03030303u;
        code4 = c2 ^ ((c2 >> 1) & 0x01010101u);
        const uint32_t exp4 = __builtin_amdgcn_perm(0u, 0x54474341u, code4);
        diff4 = u4 ^ exp4;
        ccode4 = code4 ^ 0x03030303u;                                // complement digits
      }
      uint32_t okmask = 0xFu;                                        // windows ending at base q that may be emitted
      uint64_t tq[4];                                                // PR only: the threshold in force at each base
      if (PR) { tq[0] = lthr; tq[1] = lthr; tq[2] = lthr; tq[3] = lthr; }
      if (!((PK || diff4 == 0) && i0 - g_lo < g_span)) {
        if (PK && i0 < 256u && ((dmask >> (i0 >> 2)) & 1ull)) {
          // a dirty group: its four bytes again, from global memory, for the per-base validity below
          uint32_t d = 0;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const uint64_t at = p0 + i0 + (uint32_t)q;
            if (at < b.len) d |= (uint32_t)b.seq[at] << (8 * q);
          }
          const uint32_t u4 = d & 0xDFDFDFDFu;
          uint32_t actg;                                             // (a scalar register: see the staging loop)
          asm("s_mov_b32 %0, 0x47544341" : "=s"(actg));
          diff4 = u4 ^ __builtin_amdgcn_perm(0u, actg, (u4 >> 1) & 0x03030303u);   // as the staging lanes check
        }
        // ---- not clean (rare): base by base, exactly the reference's conditions
        okmask = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint32_t i = i0 + q;
          uint32_t bad = (diff4 >> (8 * q)) & 0xffu;
          if (i >= lim) {
            // at or past the end of the record's valid part: find where base p0+i belongs
            const uint64_t qpos = p0 + i;
            if (multi) {
              while (rec + 1 < b.nrec && qpos >= b.starts[rec + 1]) { rec++; vstart = i; }
              cur_end = b.vends ? b.vends[rec] : b.starts[rec + 1];
              if (PR) lthr = hp.thr_rec[rec];
            }
            if (qpos >= cur_end) { bad = 1; lim = i + 1; }
            else lim = (cur_end - p0) > 0xfffffffeull ? 0xffffffffu : (uint32_t)(cur_end - p0);
          }
          if (bad) vstart = i + 1;
          if (kHash) {
            const bool ok = (i + 1 >= vstart + (uint32_t)K) && (i < hi_ok);
            okmask |= ok ? (1u << q) : 0u;
            if (PR) tq[q] = lthr;
          }
        }
        set_clean_window(!kHash, i0 + 4);
      }
#pragma unroll
      for (int g0b = 0; g0b < 4; g0b += HB) {
        uint32_t X[HB][L];
#pragma unroll
        for (int q = 0; q < HB; q++) {
          const int bb = g0b + q;
          const uint32_t code = PK ? (w >> (2 * bb)) & 3u : (code4 >> (8 * bb)) & 3u;
          const uint32_t ccode = PK ? (wc >> (2 * bb)) & 3u : (ccode4 >> (8 * bb)) & 3u;
          if (kRoll31) {
            // (L == 2: limb 0 needs no mask; the shift amounts are constants)
            const uint32_t fhu = __builtin_amdgcn_alignbit(w >> 2, fa1, 2 * bb + 2);   // top bits: the next base
            fle[0] = __builtin_amdgcn_alignbit(fa1, fa0, 2 * bb + 2);
            fle[L - 1] = fhu & MASK[L - 1];
            cf[0] = __builtin_amdgcn_alignbit(cs0, wr, 30 - 2 * bb);
            cf[L - 1] = __builtin_amdgcn_alignbit(cs1, cs0, 30 - 2 * bb) & MASK[L - 1];
            if (bb == 3) { fa0 = fle[0]; fa1 = fhu; cs0 = cf[0]; cs1 = cf[L - 1]; }
          } else {
          // cf = ((cf << 2) | (3 - code)) & MASK ; fle = (fle >> 2) | code << (2K-2)   (limb-wise)
#pragma unroll
          for (int li = L - 1; li > 0; li--) cf[li] = __builtin_amdgcn_alignbit(cf[li], cf[li - 1], 30) & MASK[li];
          cf[0] = ((cf[0] << 2) | ccode) & MASK[0];
#pragma unroll
          for (int li = 0; li < L - 1; li++) fle[li] = __builtin_amdgcn_alignbit(fle[li + 1], fle[li], 2);
          fle[L - 1] >>= 2;
#pragma unroll
          for (int li = 0; li < L; li++)
            if (li == top_limb) fle[li] |= code << top_sh;
          }
          if (kHash) {
            // canonical strand: kmer < rc  <=>  fle < cf (see above), decided from the top limb down
            bool fwd = false;
            if (kMinF64) {
              // Both windows are below 2^62 (k <= 31): as IEEE doubles they are non-negative, never NaN or infinite (bit 62,
              // the exponent's top bit, is clear), and ordered like the integers, so the smaller window is ONE v_min_f64
              // instead of v_cmp_lt_u64 + two v_cndmask_b32.  A window below 2^52 is a DENORMAL: the result is the operand
              // unchanged only because the kernels run with 64-bit denormals kept (float_denorm_mode_16_64 = 3, the
              // compiler's default for this target; -fno-fast-math, see csrc/Makefile).  Inline asm, not fmin(): no
              // canonicalising step.  With denormals flushed every k = 21 window would hash as zero:
              // tests/test_gpu_dna_strand_min.py fails at once.
              uint64_t x;
              asm("v_min_f64 %0, %1, %2" : "=v"(x) : "v"(((uint64_t)fle[1] << 32) | fle[0]), "v"(((uint64_t)cf[1] << 32) | cf[0]));
              X[q][0] = (uint32_t)x; X[q][L - 1] = (uint32_t)(x >> 32);
            } else if (L == 2) {
              fwd = (((uint64_t)fle[1] << 32) | fle[0]) < (((uint64_t)cf[1] << 32) | cf[0]);
            } else {
              bool decided = false;
#pragma unroll
              for (int li = L - 1; li >= 0; li--) {
                const uint32_t f = fle[li], r = cf[li];
                if (!decided && f != r) { fwd = f < r; decided = true; }
              }
            }
            if (!kMinF64) {
#pragma unroll
              for (int li = 0; li < L; li++) X[q][li] = fwd ? fle[li] : cf[li];  // chosen strand, first base low
            }
          }
        }
        // uniform: some window of this block is complete, and some window of it ends inside a full run (windows end at
        // bases K-1 .. R+K-2; the last group of four reaches past that by (R+K-1) mod 4 bases, whose windows belong to
        // no lane and were hashed only to be masked out)
        if (kHash && i0 + g0b + HB >= (uint32_t)K && i0 + g0b < R + (uint32_t)K - 1) {
          W2 ha[HB], hb[HB];
#pragma unroll
          for (int q = 0; q < HB; q++) {
            W2 M[2 * L];
            uint32_t S[2 * L], P[2 * L];                             // FOLD: the words' product high dwords; B' of the k2 words
#pragma unroll
            for (int wi = 0; wi < 2 * L; wi++) { M[wi] = W2{0u, 0u}; S[wi] = 0u; P[wi] = 0u; }
#pragma unroll
            for (int g = 0; g < 4 * L; g++) {
              if (KT == 0 || 4 * g < K) {
                // byte offset of the group's table entry: its digits << 3 (entries are u64), masked to
                // the digits that belong to the k-mer; P1 / P2 by word parity, the partial table, or
                // (run-time k only) the zero entry
                const uint32_t xw = X[q][g >> 2];
                // byte (g & 3) of the limb, times 8, in ONE sub-dword-addressed shift (SDWA issues at full
                // rate on gfx950: 32.0 -> 30.8 ms per 10 GB).  No mask is needed, for any k: both windows are
                // zero above their 2k bits, so a partial group indexes inside its 4^nb-entry table and a
                // group past the k-mer reads entry 0 of the zero table.
                uint32_t off;                  // digits << 3 (8-byte entries), << 4 (FOLD: 16-byte entries) or << 2 (packed low dwords)
                                               // (CROSS, high half of a k2 word: << 3, the {B, B'} entries)
                if ((g & 3) == 0 && FOLD) asm("v_lshlrev_b32_sdwa %0, 4, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(off) : "v"(xw));
                else if ((g & 3) == 0) asm("v_lshlrev_b32_sdwa %0, 3, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(off) : "v"(xw));
                else if ((g & 3) == 1) asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(off) : "v"(xw));
                else if ((g & 3) == 2 && FOLD) asm("v_lshlrev_b32_sdwa %0, 4, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(off) : "v"(xw));
                else if ((g & 3) == 2) asm("v_lshlrev_b32_sdwa %0, 3, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(off) : "v"(xw));
                else if ((g & 3) == 3 && CROSS) asm("v_lshlrev_b32_sdwa %0, 3, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(off) : "v"(xw));
                else asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(off) : "v"(xw));
                const char* at = reinterpret_cast<const char*>(lut) + gbase[g] + off;
                if ((g & 1) == 0 && FOLD) {                          // low half, folded: {T, a.hi, 0}
                  // (the empty asm "uses" the pad dword: otherwise the read shrinks to a ds_read_b96, which takes 8 LDS
                  // cycles per wave where ds_read_b128 takes 4)
                  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                  u32x4 e = *reinterpret_cast<const u32x4*>(at);
                  asm("" : "+v"(e));
                  M[g >> 1] = W2{e.x, e.y};
                  S[g >> 1] = e.z;
                } else if ((g & 1) == 0) {                           // low half of the word: full product
                  const uint2 e = *reinterpret_cast<const uint2*>(at);
                  M[g >> 1] = W2{e.x, e.y};
                } else if (CROSS && (g & 2)) {                       // high half of a k2 word: {B, B'}
                  const uint2 e = *reinterpret_cast<const uint2*>(at);
                  S[g >> 1] += e.x;
                  P[g >> 1] = e.y;
                } else if (FOLD) {
                  S[g >> 1] += *reinterpret_cast<const uint32_t*>(at);      // high half: (entry << 32), low dword only
                } else {
                  M[g >> 1].hi += *reinterpret_cast<const uint32_t*>(at);   // high half: (entry << 32), low dword only
                }
              }
            }
            murmur_kmer_pre<L, FOLD, CROSS, S32, (S32 && (KT & 15) > 0) ? KT : 0>(M, S, P, K, hp.seed, seedv, ha[q], hb[q]);
          }
#pragma unroll
          for (int q = 0; q < HB; q++)
            if (open_hi_sum1<SUMF>(ha[q], hb[q]) <= (PR ? open_thr<SUMF>(tq[g0b + q]) : thr_hi1)) {   // ~1 in `scaled` windows gets here
              uint32_t om = okmask;
              asm volatile("" : "+v"(om));                  // keeps the mask test inside this rare block
              const uint64_t h = open_full(ha[q], hb[q]);
              if (h <= (PR ? tq[g0b + q] : thr) && ((om >> (g0b + q)) & 1u))
                stage_emit(stage, sink, h, hp.pos_base + p0 + (i0 + g0b + q + 1 - (uint32_t)K));
            }
        }
      }
      if (PK) { w >>= 8; wc >>= 8; }
      if (kRoll31) wr <<= 8;
    };

    set_clean_window(true, 0);
    if (kRoll31 && !PR && g_span > 24u) {
      // k = 31, packed tile, all seven warm-up groups clean (g_lo = 0 here: no dirty dword and no end of the record's valid
      // part in bases 0..27): the state the groups would leave is a function of the run's first 28 codes (29 for fa's top
      // bits), which sit in three tile dwords, and is formed directly.  q0, q1 = the codes of bases 0..15 and 16..31.
      const uint32_t d1 = tile[cq + 1 + ((cq + 1) >> (logR - 4))], d2 = tile[cq + 2 + ((cq + 2) >> (logR - 4))];
      const uint32_t q0 = __builtin_amdgcn_alignbit(d1, pcur, sh2), q1 = __builtin_amdgcn_alignbit(d2, d1, sh2);
      cq += 2; pcur = d2;
      fa0 = q0 << 6;                                                 // base 0 at bit 6 ... base 28 at bits 62..63
      fa1 = __builtin_amdgcn_alignbit(q1, q0, 26);
      const uint32_t r0 = __builtin_bitreverse32(q0), r1 = __builtin_bitreverse32(q1);
      const uint32_t c0 = ~(((r0 >> 1) & 0x55555555u) | ((r0 << 1) & 0xaaaaaaaau));   // complements, base j in bits 30-2j
      const uint32_t c1 = ~(((r1 >> 1) & 0x55555555u) | ((r1 << 1) & 0xaaaaaaaau));
      cs0 = __builtin_amdgcn_alignbit(c0, c1, 8);                    // base 27 at bits 0..1 ... base 0 at bits 54..55
      cs1 = c0 >> 8;
      w = q1 >> 24; wc = ~q1 >> 24; wr = c1 << 24;                   // the quad's last group: bases 28..31
    } else {
      for (uint32_t i0 = 0; i0 < warm_end; i0 += 4) group(i0, std::false_type{});
    }
    // (the hashing loop's counter starts at a constant on either path: it stays in a scalar register, and the tests
    // on it -- a new dword every 16 bases, the block guards -- stay uniform)
    set_clean_window(false, warm_end);
    for (uint32_t i0 = warm_end; i0 < nsteps; i0 += 4) group(i0, std::true_type{});
    }  // p0 < range_hi

    // ---- flush the staged candidates: ONE global atomic per tile, coalesced stores
    stage_flush(stage, sink, tid, THREADS);
    // (uniform: read into a scalar register, or everything derived from the tile number would move to vector registers)
    if (!PR && tile_ctr) tix = (uint64_t)gridDim.x + (uint32_t)__builtin_amdgcn_readfirstlane((int)st_ctl[4]);
    else tix += gridDim.x;
  }
}

// ---------------------------------------------------------------------------------
// DNA arm, any ksize: one lane per k-mer start position
__global__ __launch_bounds__(256) void k_dna_generic(SeqBatch b, HashParams hp, CandSink sink) {
  const uint64_t K = hp.ksize;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t p = hp.range_lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < hp.range_hi;
       p += stride) {
    uint64_t end = b.vend0, thr = hp.thr;
    if (b.starts) {
      uint32_t r = find_record(b.starts, b.nrec, p);
      end = b.vends ? b.vends[r] : b.starts[r + 1];
      if (hp.thr_rec) thr = hp.thr_rec[r];
    }
    if (p + K > end || p + K < p) continue;
    const uint8_t* s = b.seq + p;
    bool ok = true, decided = false, fwd = true;
    for (uint64_t i = 0; i < K; i++) {
      uint32_t f = upper(s[i]);
      if (!(f == 'A' || f == 'C' || f == 'G' || f == 'T')) { ok = false; break; }
      if (!decided) {
        uint32_t t = upper(s[K - 1 - i]);
        uint32_t rc = t == 'A' ? 'T' : t == 'T' ? 'A' : t == 'C' ? 'G' : t == 'G' ? 'C' : t;
        if (f != rc) { fwd = f < rc; decided = true; }
      }
    }
    if (!ok) continue;
    Mm3Stream st(hp.seed);
    for (uint64_t i = 0; i < K; i++) {
      uint32_t c;
      if (fwd) c = upper(s[i]);
      else {
        uint32_t t = upper(s[K - 1 - i]);
        c = t == 'A' ? 'T' : t == 'T' ? 'A' : t == 'C' ? 'G' : 'C';
      }
      st.push(c);
    }
    uint64_t h = st.finish();
    if (h <= thr) emit(sink, h, hp.pos_base + p);
  }
}

// ---------------------------------------------------------------------------------
// force == false: the smallest position of a byte outside [ACGTacgt] per record (atomicMin into vends, pre-filled with
// the record ends).  16 bytes per lane per step, aligned, validity four bytes at a time as in k_dna_rolling (10 GB in
// ~3 ms; the byte-at-a-time version took 11).
__global__ __launch_bounds__(256) void k_first_invalid(SeqBatch b, uint64_t* __restrict__ vends) {
  const uintptr_t p0 = (uintptr_t)b.seq, pa = p0 & ~(uintptr_t)15;
  const uint64_t head = p0 - pa;
  const uint64_t nch = (head + b.len + 15) >> 4;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nch; c += stride) {
    const uint4 v = *reinterpret_cast<const uint4*>(pa + (c << 4));
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t u4 = w[k] & 0xDFDFDFDFu;
      const uint32_t c2 = (u4 >> 1) & 0x03030303u;
      const uint32_t code4 = c2 ^ ((c2 >> 1) & 0x01010101u);
      const uint32_t diff4 = u4 ^ __builtin_amdgcn_perm(0u, 0x54474341u, code4);
      if (diff4 == 0) continue;
      for (int j = 0; j < 4; j++) {
        if (((diff4 >> (8 * j)) & 0xffu) == 0) continue;
        const uint64_t at = (c << 4) + 4 * k + j;            // offset from pa
        if (at < head || at - head >= b.len) continue;       // a byte of the 16-byte granule outside the batch
        const uint64_t q = at - head;
        const uint32_t r = b.starts ? find_record(b.starts, b.nrec, q) : 0;
        atomicMin((unsigned long long*)&vends[r], (unsigned long long)q);
      }
    }
  }
}
// the first record, in order, that is at least ksize long and whose valid part ends before its end (UINT64_MAX: none)
__global__ __launch_bounds__(256) void k_first_bad_record(const uint64_t* __restrict__ starts, const uint64_t* __restrict__ vends,
                                                          uint32_t nrec, uint32_t ksize, unsigned long long* __restrict__ out) {
  unsigned long long best = ~0ull;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrec; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t st = starts[r], en = starts[r + 1];
    if (vends[r] < en && en - st >= ksize && r < best) best = r;
  }
  for (int off = 32; off; off >>= 1) {
    const unsigned long long o = __shfl_down(best, off);
    best = o < best ? o : best;
  }
  if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(out, best);
}

}  // namespace

// ---------------------------------------------------------------------------------
// launchers

// launch geometry of the rolling kernel: 512 lanes, runs of 128 positions, two hashes per block.
// Other geometries exist only in experiment builds (-DSMH_EXPERIMENTS, SOURMASH_AMD_DNA_CFG="threads,logR,hb").
struct DnaCfg { int threads, logR, hb; bool packed = true; };
static DnaCfg dna_cfg() {
  static DnaCfg cfg = [] {
    DnaCfg c{512, 7, 2};
#ifdef SMH_EXPERIMENTS
    if (const char* e = std::getenv("SOURMASH_AMD_DNA_PK")) c.packed = std::atoi(e) != 0;     // 0: the byte tile (A/B)
#endif
#ifdef SMH_EXPERIMENTS
    if (const char* e = std::getenv("SOURMASH_AMD_DNA_CFG")) {
      int t = 0, r = 0, h = 0;
      if (sscanf(e, "%d,%d,%d", &t, &r, &h) == 3 && (t == 256 || t == 512) && r >= 5 && r <= 7 &&
          (h == 1 || h == 2 || h == 4)) c = DnaCfg{t, r, h, false};
    }
#endif
    return c;
  }();
  return cfg;
}

// One launch of a k_dna_rolling instantiation over `ntiles` tiles: the grid is what is resident at once; with more tiles
// than that the workgroups take their further tiles from a counter word (Device::tile_counter, zeroed in stream order in
// front of the timed launch).  Device::count records which way a launch went (dna_tiles_dynamic / dna_tiles_static).
// seed32: the instantiation is the one for seeds below 2^32 (k_dna_rolling's S32), recorded as dna_seed32 / dna_seed64.
// The per-record kernels have no dynamic path (see the kernel's tile loop) and keep the launch they had: 8 workgroups per
// CU, four of them resident, tiles split statically -- measured on the bench kernel, a static split over just the resident
// workgroups is SLOWER than over more, smaller shares (profiles/r09_dna_schedule.json, grid_sweep).
template <class Kernel>
static void launch_rolling_tiles(Kernel kernel, int threads, bool per_record, bool seed32, const SeqBatch& b, const HashParams& p, const CandSink& sink,
                                 uint64_t ntiles, size_t lds, int logR, uint32_t stage_cap, Device& dev, hipStream_t s) {
  uint64_t grid = per_record ? (uint64_t)dev.cu_count() * 8 : resident_workgroups(kernel, threads, lds, dev);
  bool dynamic = !per_record && ntiles > grid && ntiles < (1ull << 31);
#ifdef SMH_EXPERIMENTS
  // "n": n workgroups per CU, tiles split statically (the grid before the residency query was cu_count * 8); "static": the
  // resident grid with the static split
  if (const char* e = per_record ? nullptr : std::getenv("SOURMASH_AMD_DNA_GRID")) {
    if (std::atoi(e) > 0) grid = (uint64_t)dev.cu_count() * (uint64_t)std::atoi(e);
    dynamic = false;
  }
#endif
  if (grid > ntiles) grid = ntiles;
  uint32_t* ctr = dynamic ? dev.tile_counter(s) : nullptr;
  dev.count(dynamic ? "dna_tiles_dynamic" : "dna_tiles_static");
  dev.count(seed32 ? "dna_seed32" : "dna_seed64");
  dev.prof_begin(s);
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds, s, b, p, sink, logR, stage_cap, ctr);
}

template <int KT, int L>
static void launch_rolling(const SeqBatch& b, const HashParams& p, const CandSink& sink, uint64_t ntiles, size_t lds,
                           int logR, uint32_t stage_cap, const DnaCfg& c, Device& dev, hipStream_t s) {
#define SMH_LAUNCH_K(T, ...) launch_rolling_tiles(k_dna_rolling<KT, T, __VA_ARGS__>, T, p.thr_rec != nullptr, false, b, p, sink, ntiles, lds, logR, stage_cap, dev, s)
#define SMH_LAUNCH(T, H) SMH_LAUNCH_K(T, H, L)
  if (p.thr_rec) {   // per-record thresholds: default geometry only
    if (c.packed) SMH_LAUNCH_K(512, 2, L, true, true);
    else SMH_LAUNCH_K(512, 2, L, true);
    return;
  }
  if (c.packed) {    // the product geometry: 512 lanes, two hashes per block, the tile packed to two bits per base
#ifdef SMH_EXPERIMENTS
    if (const char* e = std::getenv("SOURMASH_AMD_DNA_PKV")) {     // "minw,hb" of the packed kernel (A/B)
      int mw = 0, hb = 0;
      if (sscanf(e, "%d,%d", &mw, &hb) == 2) {
#define SMH_PKV(M_, H_) if (mw == M_ && hb == H_) { SMH_LAUNCH_K(512, H_, L, false, true, M_); return; }
        SMH_PKV(8, 1) SMH_PKV(7, 1) SMH_PKV(6, 1) SMH_PKV(5, 1) SMH_PKV(4, 1) SMH_PKV(8, 2) SMH_PKV(6, 2) SMH_PKV(5, 2) SMH_PKV(4, 2) SMH_PKV(8, 4) SMH_PKV(6, 4)
#undef SMH_PKV
      }
    }
#endif
    // (six waves per SIMD, one hash per block: 80 vector registers keep the scalar values out of vector lanes; 27.2 against
    // 27.6 ms per 10 GB with eight waves and two hashes per block, profiles/r04_pmc_dna_rolling.json "variants_measured")
    // (two limbs: a seed below 2^32 -- every seed sourmash passes -- has its own instantiation, see murmur_kmer_pre)
    if constexpr (L == 2) {
      if ((p.seed >> 32) == 0) {
        launch_rolling_tiles(k_dna_rolling<KT, 512, 1, L, false, true, 6, true>, 512, false, true, b, p, sink, ntiles, lds, logR, stage_cap, dev, s);
        return;
      }
    }
    SMH_LAUNCH_K(512, 1, L, false, true, 6);
    return;
  }
#ifdef SMH_EXPERIMENTS
  if (c.threads == 512) { if (c.hb == 4) SMH_LAUNCH(512, 4); else if (c.hb == 2) SMH_LAUNCH(512, 2); else SMH_LAUNCH(512, 1); }
  else { if (c.hb == 4) SMH_LAUNCH(256, 4); else if (c.hb == 2) SMH_LAUNCH(256, 2); else SMH_LAUNCH(256, 1); }
#else
  SMH_LAUNCH(512, 2);
#endif
#undef SMH_LAUNCH
#undef SMH_LAUNCH_K
}

void launch_dna_hash(const SeqBatch& b_in, const HashParams& p, const CandSink& sink, Device& dev,
                     hipStream_t s, bool force_generic) {
  if (p.range_hi <= p.range_lo) return;
  const uint64_t span = p.range_hi - p.range_lo;
  if (p.ksize >= 1 && p.ksize <= 128 && !force_generic) {
    // run length per lane: long runs amortise the k-1 warm-up bases; short inputs use short
    // runs so that the launch still covers the chip
    DnaCfg c = dna_cfg();
    if (p.thr_rec) { c.threads = 512; c.logR = 7; c.hb = 2; }     // the per-record variant exists in one geometry
    int logR = c.logR;
    while (logR > 5 && (span >> logR) < (uint64_t)dev.cu_count() * c.threads * 2) logR--;
    const uint64_t tile = (uint64_t)c.threads << logR;
    const uint64_t ntiles = (span + tile - 1) / tile;
    const SeqBatch b = with_tile_records(b_in, 0, p.range_lo, tile, ntiles, dev, s);
    const int limbs = p.ksize <= 32 ? 2 : (p.ksize <= 64 ? 4 : 8);
    const uint32_t x_bytes = (uint32_t)tile + 16 * limbs + 96;
    // LDS stage for the survivors of one tile: twice the expectation under a uniform hash, within
    // [128, 2048] entries; anything beyond goes straight to the global sink
    const uint64_t thr = p.thr;
    long double expect = (long double)tile * (((long double)thr + 1.0L) / 18446744073709551616.0L);
    uint32_t stage_cap = expect * 2.0L + 64.0L > 2048.0L ? 2048u : (uint32_t)(expect * 2.0L + 64.0L);
    if (stage_cap < 128) stage_cap = 128;
    size_t lds = 4 * kDnaCtlDwords + (size_t)stage_cap * 8 * (sink.pos ? 2 : 1) + x_bytes +   // dynamic part; the tables are static LDS
                 4 * ((x_bytes >> logR) + 2);
    if (c.packed) {
      // two bits per base + a pad dword per run + a dirty bit per source dword (the kernel's nchunks_cap)
      const uint32_t ncap = (15u + (uint32_t)tile + 16u * (uint32_t)limbs + 8u + 15u + 32u) >> 4;
      lds = 4 * kDnaCtlDwords + (size_t)stage_cap * 8 * (sink.pos ? 2 : 1) + 4 * (size_t)(ncap + (ncap >> (logR - 4)) + 2) + 4 * (size_t)((ncap >> 3) + 8);
    }
    // (the grid and how the tiles are handed out: launch_rolling_tiles.  The bench kernel -- k = 31, packed tile, 69 vector
    // registers (71 for a seed at or above 2^32), ~35 KB of LDS -- has three 512-lane workgroups per CU resident.)
    if (p.ksize == 31) launch_rolling<31, 2>(b, p, sink, ntiles, lds, logR, stage_cap, c, dev, s);
    else if (p.ksize == 21) launch_rolling<21, 2>(b, p, sink, ntiles, lds, logR, stage_cap, c, dev, s);
    else if (p.ksize == 51) launch_rolling<51, 4>(b, p, sink, ntiles, lds, logR, stage_cap, c, dev, s);
    else if (p.ksize <= 32) launch_rolling<0, 2>(b, p, sink, ntiles, lds, logR, stage_cap, c, dev, s);
    else if (p.ksize <= 64) launch_rolling<0, 4>(b, p, sink, ntiles, lds, logR, stage_cap, c, dev, s);
    else launch_rolling<0, 8>(b, p, sink, ntiles, lds, logR, stage_cap, c, dev, s);
    HIP_CHECK(hipGetLastError());
    dev.prof_end("dna_rolling", s);
  } else {
    dev.prof_begin(s);
    hipLaunchKernelGGL(k_dna_generic, dim3(sketch_grid(span, 256, dev.cu_count() * 16)), dim3(256), 0, s,
                       b_in, p, sink);
    HIP_CHECK(hipGetLastError());
    dev.prof_end("dna_generic", s);
  }
}

// out[0] = records of at least ksize bases, out[1] = positions of the protein arm's six-frame layout (2 (len - 2) per such
// record: len / 3 + (len - 1) / 3 + (len - 2) / 3 == len - 2).  A batch of reads has tens of millions of records; a
// host pass over their offsets costs more than hashing them.
__global__ __launch_bounds__(256) void k_record_stats(const uint64_t* __restrict__ starts, uint32_t nrec, uint32_t ksize,
                                                      unsigned long long* __restrict__ out) {
  unsigned long long nlong = 0, total = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrec; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t len = starts[r + 1] - starts[r];
    if (len >= ksize) {
      nlong++;
      if (len >= 2) total += 2 * (len - 2);
      else for (uint32_t f = 0; f < 3; f++) total += len >= f ? 2 * ((len - f) / 3) : 0;
    }
  }
  for (int off = 32; off; off >>= 1) { nlong += __shfl_down(nlong, off); total += __shfl_down(total, off); }
  if ((threadIdx.x & 63) == 0 && (nlong | total)) { atomicAdd(&out[0], nlong); atomicAdd(&out[1], total); }
}
void launch_record_stats(const uint64_t* starts, uint32_t nrec, uint32_t ksize, uint64_t* out2, hipStream_t s) {
  HIP_CHECK(hipMemsetAsync(out2, 0, 16, s));
  hipLaunchKernelGGL(k_record_stats, dim3(sketch_grid(nrec, 256, 2048)), dim3(256), 0, s, starts, nrec, ksize,
                     reinterpret_cast<unsigned long long*>(out2));
  HIP_CHECK(hipGetLastError());
}

void launch_first_bad_record(const uint64_t* starts, const uint64_t* vends, uint32_t nrec, uint32_t ksize, uint64_t* out, hipStream_t s) {
  HIP_CHECK(hipMemsetAsync(out, 0xff, 8, s));
  hipLaunchKernelGGL(k_first_bad_record, dim3(sketch_grid(nrec, 256, 2048)), dim3(256), 0, s, starts, vends, nrec, ksize,
                     reinterpret_cast<unsigned long long*>(out));
  HIP_CHECK(hipGetLastError());
}

void launch_first_invalid(const SeqBatch& b, uint64_t* vends_out, hipStream_t s) {
  if (b.len == 0) return;
  hipLaunchKernelGGL(k_first_invalid, dim3(sketch_grid(b.len + 32, 256 * 16, 8192)), dim3(256), 0, s, b,
                     vends_out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace smh
