// murmur_device.hpp -- device code shared by the sketch kernels' translation units (sketch_kernels.hip,
// sketch_dna_kernels.hip, sketch_protein_kernels.hip, sketch_amino_kernels.hip): MurmurHash3 x64_128 in 64-bit integers
// (whole blocks and the byte-at-a-time stream), the same arithmetic on explicit 32-bit halves (W2), the open digest with
// its filter, and murmur64 of a string of at most 16 bytes (the fused protein kernel and the amino-acid kernel).  What only
// one arm uses is in that arm's file.  No state: everything is __device__ __forceinline__ or constexpr.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smh {

// ---------------------------------------------------------------------------------
// MurmurHash3 x64_128 pieces (crate murmurhash3 ~0.0.5 as called at reference src/lib.rs:33-35)
constexpr uint64_t kC1 = 0x87c37b91114253d5ULL;
constexpr uint64_t kC2 = 0x4cf5ad432745937fULL;

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t fmix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}
__device__ __forceinline__ uint64_t mix_k1(uint64_t k1) { k1 *= kC1; k1 = rotl64(k1, 31); k1 *= kC2; return k1; }
__device__ __forceinline__ uint64_t mix_k2(uint64_t k2) { k2 *= kC2; k2 = rotl64(k2, 33); k2 *= kC1; return k2; }
__device__ __forceinline__ void mm3_block(uint64_t& h1, uint64_t& h2, uint64_t k1, uint64_t k2) {
  h1 ^= mix_k1(k1);
  h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
  h2 ^= mix_k2(k2);
  h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
}
__device__ __forceinline__ uint64_t mm3_finish(uint64_t h1, uint64_t h2, uint64_t len) {
  h1 ^= len; h2 ^= len;
  h1 += h2; h2 += h1;
  h1 = fmix64(h1); h2 = fmix64(h2);
  return h1 + h2;  // first word of the digest
}

// byte-at-a-time front end for strings of any length
struct Mm3Stream {
  uint64_t h1, h2, k1, k2;
  uint32_t n;
  __device__ __forceinline__ explicit Mm3Stream(uint64_t seed) : h1(seed), h2(seed), k1(0), k2(0), n(0) {}
  __device__ __forceinline__ void push(uint32_t b) {
    uint32_t r = n & 15u;
    if (r < 8) k1 |= (uint64_t)b << (8 * r);
    else k2 |= (uint64_t)b << (8 * (r - 8));
    n++;
    if ((n & 15u) == 0) { mm3_block(h1, h2, k1, k2); k1 = 0; k2 = 0; }
  }
  __device__ __forceinline__ uint64_t finish() {
    uint32_t rem = n & 15u;
    if (rem > 8) h2 ^= mix_k2(k2);
    if (rem > 0) h1 ^= mix_k1(k1);
    return mm3_finish(h1, h2, n);
  }
};

// The hash runs on explicit 32-bit halves.  Issue rates on gfx950 (tools/instr_rate.hip,
// profiles/r01_instr_rates.txt): two-operand VALU forms ~100 lanes/clk/CU, everything with three
// operands (v_alignbit, v_add3, v_lshl_add, v_bfe, v_perm), every 32-bit multiply and v_mad_u64_u32
// ~59 -- so the code below is written to need few of the latter: a 64 x 64 -> 64 multiply by a
// constant is one v_mad_u64_u32 + two v_mul_lo_u32 + one v_add3, a 64-bit rotate two v_alignbit,
// `k ^= k >> 33` two plain ops on the halves, and nothing is zero-extended into register pairs.
struct W2 { uint32_t lo, hi; };
__device__ __forceinline__ W2 w2_rotl(W2 x, int r) {   // 0 < r < 64, r != 32
  if (r < 32) return {__builtin_amdgcn_alignbit(x.lo, x.hi, 32 - r), __builtin_amdgcn_alignbit(x.hi, x.lo, 32 - r)};
  return {__builtin_amdgcn_alignbit(x.hi, x.lo, 64 - r), __builtin_amdgcn_alignbit(x.lo, x.hi, 64 - r)};
}
__device__ __forceinline__ W2 w2_mul(W2 x, uint64_t c) {
  const uint32_t cl = (uint32_t)c, ch = (uint32_t)(c >> 32);
  // three v_mad_u64_u32 and one add: t = x.hi*cl; u = x.lo*ch + t (its low dword is the whole cross
  // term); p = x.lo*cl; high dword = p.hi + u.lo.  (The compiler's own choice -- one v_mad_u64_u32,
  // two v_mul_lo_u32 and a v_add3 -- is four half-rate instructions; measured 32.6 -> 32.0 ms per 10 GB.)
  // (Three separate asm statements on purpose.  The scheduler tends to put u right behind t, which
  // costs a wait state (s_nop) per multiply; pinning the order t, p, u inside one statement removes
  // those and is nevertheless 1-2 % slower -- the padding is hidden by the other waves, the lost
  // scheduling freedom is not.  Measured on both kernels, profiles/r02_dna_kernel_steps.txt.)
  uint64_t t, u, p, cy;
  asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(t), "=s"(cy) : "v"(x.hi), "s"(cl));
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(u), "=s"(cy) : "v"(x.lo), "s"(ch), "v"(t));
  asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(p), "=s"(cy) : "v"(x.lo), "s"(cl));
  // (the add as asm too: left to the compiler it sometimes becomes a 64-bit add of p and {0, u.lo} -- two moves
  // to build the pair and a half-rate v_lshl_add_u64)
  uint32_t hi;
  asm("v_add_u32 %0, %1, %2" : "=v"(hi) : "v"((uint32_t)(p >> 32)), "v"((uint32_t)u));
  return {(uint32_t)p, hi};
}
__device__ __forceinline__ W2 w2_xor(W2 a, W2 b) { return {a.lo ^ b.lo, a.hi ^ b.hi}; }
// 64-bit values the compiler must treat as whole register pairs (an empty asm hides how they were
// put together): otherwise it splits a + b into zero-extended halves, moves and a v_add3
__device__ __forceinline__ uint64_t w2_pair(W2 a) {
  uint64_t v = ((uint64_t)a.hi << 32) | a.lo;
  asm("" : "+v"(v));
  return v;
}
__device__ __forceinline__ W2 w2_split(uint64_t v) { return {(uint32_t)v, (uint32_t)(v >> 32)}; }
__device__ __forceinline__ W2 w2_add(W2 a, W2 b) { return w2_split(w2_pair(a) + w2_pair(b)); }   // one v_lshl_add_u64
// h1 += h2; h2 += h1 (each value becomes a whole pair once)
__device__ __forceinline__ void w2_cross_add(W2& h1, W2& h2) {
  uint64_t a = w2_pair(h1), b = w2_pair(h2);
  a += b; b += a;
  h1 = w2_split(a); h2 = w2_split(b);
}
// x * 5 + c as (x << 2) + x, then + c: two v_lshl_add_u64
__device__ __forceinline__ W2 w2_mul5_add(W2 x, uint64_t c) {
  const uint64_t v = w2_pair(x);
  uint64_t t;
  asm("v_lshl_add_u64 %0, %1, 2, %1" : "=v"(t) : "v"(v));   // (left to itself the compiler multiplies by 5: two v_mad_u64_u32 and two moves)
  return w2_split(t + c);
}
// The open digest.  After `h1 += h2; h2 += h1` the digest is h = fmix(h1) + fmix(h2).  The sketch kernels stop each
// fmix in front of its last multiply: ka = w2_fmix_pre(h1), kb = w2_fmix_pre(h2); with C = fmix's second constant,
// a = ka * C, b = kb * C and h = (a ^ a >> 33) + (b ^ b >> 33) = open_full(ka, kb).  Whether h can be <= a threshold is
// settled by high dwords alone (open_hi_sum1 against open_thr): the windows that cannot pass -- all but ~1/scaled of
// them -- never form the two products, the xor-shifts or the 64-bit sum.
// The filter's threshold, open_thr<SUM>(thr), for the value open_hi_sum1<SUM>(ka, kb) forms (see there); both tests are
// supersets of the passing windows (exact test: open_full() <= thr).
//   SUM:  E = hi32((ka + kb) * C) + 1 (mod 2^32) and E - h.hi is 0, 1 or 2, so h <= thr needs E <= thr.hi + 2.  That sum
//         must not wrap: for thr.hi >= 0xfffffffd the threshold saturates to all ones and everything passes.
//   !SUM: F = a.hi + b.hi + 1 (mod 2^32) and h.hi is F - 1 or F, so h <= thr needs F <= thr.hi + 1; everything when
//         thr.hi is all ones.
template <bool SUM>
__device__ __forceinline__ uint32_t open_thr(uint64_t thr) {
  const uint32_t hi = (uint32_t)(thr >> 32);
  if (SUM) return hi >= 0xfffffffdu ? 0xffffffffu : hi + 2u;
  return hi == 0xffffffffu ? hi : hi + 1u;
}
__device__ __forceinline__ uint64_t open_finish(W2 a, W2 b) {
  a.lo ^= a.hi >> 1; b.lo ^= b.hi >> 1;
  return ((((uint64_t)a.hi << 32) | a.lo) + (((uint64_t)b.hi << 32) | b.lo));
}
// a + b as ONE v_lshl_add_u64 that leaves both operands intact (w2_add hides its operands behind an empty asm that
// "modifies" them, which costs a v_mov_b64 when an operand is still needed afterwards)
__device__ __forceinline__ W2 w2_add_keep(W2 a, W2 b) {
  uint64_t r;
  asm("v_lshl_add_u64 %0, %1, 0, %2" : "=v"(r) : "v"(((uint64_t)a.hi << 32) | a.lo), "v"(((uint64_t)b.hi << 32) | b.lo));
  return w2_split(r);
}
constexpr uint64_t kFmixC2 = 0xc4ceb9fe1a85ec53ULL;
__device__ __forceinline__ W2 w2_fmix_pre(W2 k) {
  k.lo ^= k.hi >> 1;                                   // k ^= k >> 33
  k = w2_mul(k, 0xff51afd7ed558ccdULL);
  k.lo ^= k.hi >> 1;
  return k;
}
// What the filter compares with open_thr<SUM>.  The high dword of x * C is mul_hi(x.lo, C.lo) + x.lo * C.hi + x.hi * C.lo
// (mod 2^32); the cross terms chain through the addends of v_mad_u64_u32 (only the low dword of each is used; the first
// addend is the + 1).
//   SUM:  multiplication distributes over the sum, (ka + kb) * C == a + b (mod 2^64), so ONE product's high dword stands
//         for both: with d = (ka + kb) * C, d.hi = a.hi + b.hi + cy (cy: the carry of a.lo + b.lo), while
//         h.hi = a.hi + b.hi + cy' (cy': the carry of the two xor-shifted low dwords; `k ^= k >> 33` changes the low
//         dword only).  E = d.hi + 1 (mod 2^32), hence E - h.hi = 1 + cy - cy' is 0, 1 or 2.  One 64-bit add that keeps
//         ka and kb (the rare block needs them), two mads, one mul_hi and one 32-bit add.
//   !SUM: F = a.hi + b.hi + 1 from both products' high dwords: four chained mads, two mul_hi, one v_add3.  Three
//         slow-class instructions more; kept for the kernels whose registers the sum's pair does not fit (k_dna_rolling,
//         SUMF).  k_amino_tiled tests the same F on products it forms in full.
template <bool SUM>
__device__ __forceinline__ uint32_t open_hi_sum1(W2 ka, W2 kb) {
  const uint32_t cl = (uint32_t)kFmixC2, ch = (uint32_t)(kFmixC2 >> 32);
  uint64_t s0, s1, s2, s3, cy;
  if (SUM) {
    const W2 s = w2_add_keep(ka, kb);
    asm("v_mad_u64_u32 %0, %1, %2, %3, 1" : "=v"(s0), "=s"(cy) : "v"(s.hi), "s"(cl));
    asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(s1), "=s"(cy) : "v"(s.lo), "s"(ch), "v"(s0));
    uint32_t e;   // (as asm so that it stays a 32-bit add, see w2_mul)
    asm("v_add_u32 %0, %1, %2" : "=v"(e) : "v"((uint32_t)s1), "v"(__umulhi(s.lo, cl)));
    return e;
  }
  asm("v_mad_u64_u32 %0, %1, %2, %3, 1" : "=v"(s0), "=s"(cy) : "v"(ka.hi), "s"(cl));
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(s1), "=s"(cy) : "v"(ka.lo), "s"(ch), "v"(s0));
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(s2), "=s"(cy) : "v"(kb.hi), "s"(cl), "v"(s1));
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(s3), "=s"(cy) : "v"(kb.lo), "s"(ch), "v"(s2));
  return (uint32_t)s3 + __umulhi(ka.lo, cl) + __umulhi(kb.lo, cl);
}
__device__ __forceinline__ uint64_t open_full(W2 ka, W2 kb) { return open_finish(w2_mul(ka, kFmixC2), w2_mul(kb, kFmixC2)); }

// murmur64 of a W-byte string, 1 <= W <= 16: no full block, k1 = bytes 0..7, k2 = bytes 8..W-1 (reference
// src/lib.rs:33-35 on aa.windows()).  k1c1 = k1 * c1 is handed in (the two strands get it differently, see
// k_protein_fused); k2 = the bytes past the eighth as they are; the digest is left open: (a, b) with h = open_full(a, b).
// W == 9: k2 is one byte, so its whole contribution -- seed ^ mix_k2(byte) ^ W -- comes from a table (h2_ready).
template <int W>
__device__ __forceinline__ void murmur_short(W2 k1c1, W2 k2, W2 seedw /* seed ^ W, in vector registers */, uint64_t h2_ready, W2& a, W2& b) {
  W2 h1 = seedw, h2{(uint32_t)h2_ready, (uint32_t)(h2_ready >> 32)};
  if (W != 9) {
    h2 = seedw;
    if (W > 8) h2 = w2_xor(h2, w2_mul(w2_rotl(w2_mul(k2, kC2), 33), kC1));
  }
  h1 = w2_xor(h1, w2_mul(w2_rotl(k1c1, 31), kC2));
  w2_cross_add(h1, h2);
  a = w2_fmix_pre(h1); b = w2_fmix_pre(h2);
}

}  // namespace smh
