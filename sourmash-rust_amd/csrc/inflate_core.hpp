// inflate_core.hpp -- the DEFLATE decoder (RFC 1951) of one blocked-gzip member, as one source for the device kernel
// (inflate_kernels.hip) and for a plain host build (tests/c_inflate_host.cpp): the bit reader, the table builder with all
// its validity rules, the symbol decode and every bounds check (the rules are in include/sourmash_amd.h,
// "Blocked gzip").  No HIP header is needed: the qualifiers sit behind SMH_HD.
//
// What differs by build is the Sink, which only moves bytes whose positions this file has already checked:
//   lit(pos, byte)            out[pos] = byte                                   pos < isize
//   copy(pos, dist, len)      out[pos + i] = out[pos - dist + i], i ascending   1 <= dist <= pos, pos + len <= isize
//   stored(pos, src, n)       out[pos + i] = src[i]                             src[0, n) inside the payload, pos + n <= isize
//   flush()                   everything handed over so far is in `out`
// and where the tables live (Tables: LDS on the device, the stack on the host).
//
// Termination: every step of every loop either consumes at least one input bit -- taken from a payload of in_len bytes, so
// at most 8 in_len times -- or produces at least one output byte, checked against isize; a block header consumes three bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SMH_HD __host__ __device__
#define SMH_UNROLL _Pragma("unroll")
#else
#define SMH_HD
#define SMH_UNROLL
#endif

namespace smh {
namespace inflate {

// One status per member: the first rule it broke.  The values are ABI (include/sourmash_amd.h, SMH_INFLATE_*).
enum Reason : uint8_t {
  kOk = 0,
  kBlockType = 1,        // reserved block type 3
  kStoredLen = 2,        // stored LEN != ~NLEN
  kHeaderCounts = 3,     // more than 286 literal/length or more than 30 distance codes
  kRepeat = 4,           // code-length repeat with nothing to repeat, or running past the announced lengths
  kOverSubscribed = 5,   // a code set that claims more codes than its lengths leave room for
  kIncomplete = 6,       // a code set with unused codes (a literal/length or distance set of one single 1-bit code is legal)
  kNoEndOfBlock = 7,     // symbol 256 has no code
  kBadSymbol = 8,        // literal/length 286, 287, distance 30, 31, or a bit pattern no code of the set has
  kDistance = 9,         // a match reaching in front of the member's own output
  kInput = 10,           // the payload ended inside the stream
  kOutputOver = 11,      // the output would pass ISIZE
  kOutputUnder = 12,     // the stream ended with less output than ISIZE
  kLeftover = 13,        // payload bytes behind the final block
  kCrc = 14,             // CRC-32 of the output differs from the trailer's
};
constexpr uint32_t kReasons = 15;
constexpr uint32_t kMaxMember = 65536;   // the largest ISIZE of a blocked-gzip member

// The tables of one decoder.  lens: the code lengths as they are read (320) and the 19 of the code-length code behind them;
// lsym / dsym: symbols ordered by (length, symbol), the canonical order; work: 16 counters of the builder.  About 1 KiB.
struct Tables {
  uint8_t* lens;     // 344
  uint16_t* lsym;    // 288
  uint16_t* dsym;    // 32 (holds the code-length code's 19 symbols while a dynamic header is read)
  uint16_t* work;    // 16
};
constexpr uint32_t kLensBytes = 344, kLitSyms = 288, kDistSyms = 32, kWorkWords = 16;
constexpr uint32_t kTableBytes = kLensBytes + 2 * (kLitSyms + kDistSyms + kWorkWords);   // 1016

// LSB-first bit reader over in[0, len): no byte outside is read.
struct Bits {
  const uint8_t* in;
  uint32_t len, pos;   // pos: the next byte to load
  uint64_t buf;
  uint32_t cnt;        // valid bits in buf
  SMH_HD Bits(const uint8_t* p, uint32_t n) : in(p), len(n), pos(0), buf(0), cnt(0) {}
  SMH_HD void fill() {   // at least 32 bits afterwards, or everything the payload still has
    if (cnt > 32) return;
    if (len - pos >= 4) {
      const uint32_t w = (uint32_t)in[pos] | (uint32_t)in[pos + 1] << 8 | (uint32_t)in[pos + 2] << 16 | (uint32_t)in[pos + 3] << 24;
      buf |= (uint64_t)w << cnt;
      pos += 4; cnt += 32;
    } else {
      while (pos < len) { buf |= (uint64_t)in[pos++] << cnt; cnt += 8; }
    }
  }
  SMH_HD bool need(uint32_t n) { fill(); return cnt >= n; }   // n <= 32
  SMH_HD uint32_t take(uint32_t n) {                           // after need(n)
    const uint32_t v = (uint32_t)(buf & ((1ull << n) - 1));
    buf >>= n; cnt -= n;
    return v;
  }
  // drops the rest of the running byte and hands the buffered whole bytes back: pos is the next unread byte
  SMH_HD void align() {
    const uint32_t drop = cnt & 7;
    buf >>= drop; cnt -= drop;
    pos -= cnt >> 3;
    buf = 0; cnt = 0;
  }
  SMH_HD uint32_t unread_bytes() const { return len - pos + (cnt >> 3); }   // whole bytes no bit of which was consumed
};

enum BuildResult : int { kBuilt = 0, kBuiltOver = 1, kBuiltIncomplete = 2 };

// Canonical code of n lengths (0: the symbol has no code): cnt[l] = codes of length l (cnt in the caller's registers),
// sym = the coded symbols by (length, symbol).  *coded = how many symbols have a code.
SMH_HD inline int build_code(const uint8_t* lens, uint32_t n, uint16_t* cnt, uint16_t* sym, uint16_t* work, uint32_t* coded) {
  for (uint32_t l = 0; l < 16; l++) work[l] = 0;
  for (uint32_t s = 0; s < n; s++) work[lens[s] & 15] = (uint16_t)(work[lens[s] & 15] + 1);
  int32_t left = 1;
  uint32_t at = 0;
  bool over = false;
  SMH_UNROLL
  for (uint32_t l = 1; l < 16; l++) {
    const uint16_t c = work[l];
    cnt[l] = c;
    left = (left << 1) - (int32_t)c;
    if (left < 0) { over = true; left = 0; }   // (left stays small: no overflow on hostile counts)
    work[l] = (uint16_t)at;                    // where the symbols of length l start
    at += c;
  }
  cnt[0] = 0;
  *coded = at;
  if (over) return kBuiltOver;
  for (uint32_t s = 0; s < n; s++) {
    const uint32_t l = lens[s] & 15;
    if (l) { sym[work[l]] = (uint16_t)s; work[l] = (uint16_t)(work[l] + 1); }   // work[l] < at <= n: inside sym
  }
  return left > 0 ? kBuiltIncomplete : kBuilt;
}

// One symbol, a bit at a time down the canonical code.  >= 0: the symbol; -1: the payload ended; -2: no code matches.
SMH_HD inline int decode_symbol(Bits& b, const uint16_t* cnt, const uint16_t* sym) {
  b.fill();
  uint32_t code = 0, first = 0, index = 0;
  uint64_t buf = b.buf;
  const uint32_t have = b.cnt;
  SMH_UNROLL
  for (uint32_t l = 1; l < 16; l++) {
    if (l > have) return -1;
    code |= (uint32_t)(buf & 1);
    buf >>= 1;
    const uint32_t c = cnt[l];
    if (code < first + c) {          // (code >= first always)
      b.buf = buf; b.cnt = have - l;
      return sym[index + (code - first)];
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -2;
}

SMH_HD inline uint32_t length_base(uint32_t c, uint32_t* extra) {   // c = symbol - 257, 0 .. 28
  if (c < 8) { *extra = 0; return 3 + c; }
  if (c == 28) { *extra = 0; return 258; }
  const uint32_t e = (c - 4) >> 2;
  *extra = e;
  return 3 + ((4 + (c & 3)) << e);
}
SMH_HD inline uint32_t distance_base(uint32_t d, uint32_t* extra) {   // d = 0 .. 29
  if (d < 4) { *extra = 0; return 1 + d; }
  const uint32_t e = (d - 2) >> 1;
  *extra = e;
  return 1 + ((2 + (d & 1)) << e);
}
// the order in which a dynamic header stores the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
SMH_HD inline uint32_t clen_order(uint32_t i) {
  const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                      5ull << 45 | 11ull << 50 | 4ull << 55;
  const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

// The header of a dynamic block -> the two codes.  lcnt / dcnt: 16 counters each, in the caller's registers.
SMH_HD inline uint8_t read_dynamic(Bits& b, const Tables& t, uint16_t* lcnt, uint16_t* dcnt) {
  if (!b.need(14)) return kInput;
  const uint32_t nlen = b.take(5) + 257, ndist = b.take(5) + 1, ncode = b.take(4) + 4;
  if (nlen > 286 || ndist > 30) return kHeaderCounts;
  uint8_t* clens = t.lens + 320;
  for (uint32_t i = 0; i < 19; i++) clens[i] = 0;
  for (uint32_t i = 0; i < ncode; i++) {
    if (!b.need(3)) return kInput;
    clens[clen_order(i)] = (uint8_t)b.take(3);
  }
  uint16_t ccnt[16];
  uint32_t coded;
  const int r = build_code(clens, 19, ccnt, t.dsym, t.work, &coded);
  if (r == kBuiltOver) return kOverSubscribed;
  if (r == kBuiltIncomplete) return kIncomplete;      // (also a code-length code of one code, or of none)
  const uint32_t total = nlen + ndist;
  uint32_t have = 0;
  while (have < total) {                              // every trip consumes at least one bit
    const int s = decode_symbol(b, ccnt, t.dsym);
    if (s == -1) return kInput;
    if (s < 0) return kBadSymbol;                     // (cannot happen: the code is complete)
    if (s < 16) { t.lens[have++] = (uint8_t)s; continue; }
    uint32_t rep, val = 0;
    if (s == 16) {
      if (have == 0) return kRepeat;
      if (!b.need(2)) return kInput;
      val = t.lens[have - 1];
      rep = 3 + b.take(2);
    } else if (s == 17) {
      if (!b.need(3)) return kInput;
      rep = 3 + b.take(3);
    } else {
      if (!b.need(7)) return kInput;
      rep = 11 + b.take(7);
    }
    if (rep > total - have) return kRepeat;
    for (uint32_t i = 0; i < rep; i++) t.lens[have++] = (uint8_t)val;
  }
  if (t.lens[256] == 0) return kNoEndOfBlock;
  int rr = build_code(t.lens, nlen, lcnt, t.lsym, t.work, &coded);
  if (rr == kBuiltOver) return kOverSubscribed;
  if (rr == kBuiltIncomplete && !(coded == 1 && lcnt[1] == 1)) return kIncomplete;
  rr = build_code(t.lens + nlen, ndist, dcnt, t.dsym, t.work, &coded);
  if (rr == kBuiltOver) return kOverSubscribed;
  if (rr == kBuiltIncomplete && !(coded == 0 || (coded == 1 && dcnt[1] == 1))) return kIncomplete;
  return kOk;
}

// the fixed codes of RFC 1951 3.2.6 through the same builder (literal/length 286, 287 and distance 30, 31 have codes: using
// one is kBadSymbol)
SMH_HD inline void build_fixed(const Tables& t, uint16_t* lcnt, uint16_t* dcnt) {
  for (uint32_t s = 0; s < 288; s++) t.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
  uint32_t coded;
  (void)build_code(t.lens, 288, lcnt, t.lsym, t.work, &coded);
  for (uint32_t s = 0; s < 32; s++) t.lens[s] = 5;
  (void)build_code(t.lens, 32, dcnt, t.dsym, t.work, &coded);
}

// Inflates in[0, in_len) into the sink: at most isize bytes, and exactly isize for kOk.  *produced = the bytes handed to the
// sink.  The CRC is the caller's (it reads the finished output).
template <class Sink>
SMH_HD inline uint8_t inflate_member(const uint8_t* in, uint32_t in_len, uint32_t isize, const Tables& t, Sink& sink, uint32_t* produced) {
  Bits b(in, in_len);
  uint32_t pos = 0;
  uint16_t lcnt[16], dcnt[16];
  *produced = 0;
  for (;;) {
    if (!b.need(3)) return kInput;
    const uint32_t last = b.take(1), type = b.take(2);
    if (type == 3) return kBlockType;
    if (type == 0) {
      b.align();
      if (in_len - b.pos < 4) return kInput;
      const uint32_t n = (uint32_t)in[b.pos] | (uint32_t)in[b.pos + 1] << 8;
      const uint32_t nn = (uint32_t)in[b.pos + 2] | (uint32_t)in[b.pos + 3] << 8;
      b.pos += 4;
      if (n != (nn ^ 0xffffu)) return kStoredLen;
      if (n > in_len - b.pos) return kInput;
      if (n > isize - pos) return kOutputOver;
      if (n) sink.stored(pos, in + b.pos, n);
      b.pos += n; pos += n;
      *produced = pos;
    } else {
      if (type == 1) {
        build_fixed(t, lcnt, dcnt);
      } else {
        const uint8_t r = read_dynamic(b, t, lcnt, dcnt);
        if (r != kOk) return r;
      }
      for (;;) {                                     // every trip consumes at least one bit
        const int s = decode_symbol(b, lcnt, t.lsym);
        if (s == -1) return kInput;
        if (s < 0) return kBadSymbol;
        if (s < 256) {
          if (pos >= isize) return kOutputOver;
          sink.lit(pos, (uint8_t)s);
          *produced = ++pos;
          continue;
        }
        if (s == 256) break;
        if (s > 285) return kBadSymbol;
        uint32_t extra;
        uint32_t len = length_base((uint32_t)s - 257, &extra);
        if (!b.need(extra)) return kInput;
        len += b.take(extra);
        const int ds = decode_symbol(b, dcnt, t.dsym);
        if (ds == -1) return kInput;
        if (ds < 0 || ds > 29) return kBadSymbol;
        uint32_t dist = distance_base((uint32_t)ds, &extra);
        if (!b.need(extra)) return kInput;
        dist += b.take(extra);
        if (dist > pos) return kDistance;
        if (len > isize - pos) return kOutputOver;
        sink.copy(pos, dist, len);
        pos += len;
        *produced = pos;
      }
    }
    if (last) break;
  }
  sink.flush();
  if (pos < isize) return kOutputUnder;
  if (b.unread_bytes() != 0) return kLeftover;
  return kOk;
}

// --- CRC-32 (IEEE 802.3, reflected: polynomial 0xedb88320) ------------------------------------------------------------
// The register after the bytes D from state s is affine in s: run(s, D) = run(s, 0^|D|) ^ run(0, D), and run(s, 0^n) is the
// product s * x^(8n) mod P.  So the slices of a member can be run from state 0 by 64 lanes, each result shifted over the
// bytes behind its slice and the lot XOR-ed: crc = ~(shift(~0, total) ^ XOR_i shift(run(0, D_i), bytes behind slice i)).
constexpr uint32_t kCrcPoly = 0xedb88320u;
SMH_HD inline uint32_t crc_table_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
  return c;
}
SMH_HD inline uint32_t crc_run(uint32_t state, const uint8_t* p, uint32_t n, const uint32_t* table) {
  for (uint32_t i = 0; i < n; i++) state = table[(state ^ p[i]) & 0xff] ^ (state >> 8);
  return state;
}
// a * b mod P, both reflected (bit 31 is x^0)
SMH_HD inline uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int k = 0; k < 32; k++) {
    if (a & (0x80000000u >> k)) p ^= b;
    b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
// state * x^(8 n) mod P: the register after n more zero bytes
SMH_HD inline uint32_t crc_shift(uint32_t state, uint32_t n) {
  uint32_t pw = 0x80000000u, base = 0x00800000u;   // x^0, x^8
  for (int k = 0; k < 32 && n; k++) {
    if (n & 1) pw = crc_mul(pw, base);
    base = crc_mul(base, base);
    n >>= 1;
  }
  return crc_mul(state, pw);
}
// the slice of lane i of `lanes` over total bytes: [slice_begin(i), slice_begin(i + 1))
SMH_HD inline uint32_t crc_slice_begin(uint32_t total, uint32_t lanes, uint32_t i) {
  const uint32_t per = (total + lanes - 1) / lanes;
  const uint64_t at = (uint64_t)per * i;
  return at < total ? (uint32_t)at : total;
}
// lane i's term of the XOR above
SMH_HD inline uint32_t crc_lane_term(const uint8_t* out, uint32_t total, uint32_t lanes, uint32_t i, const uint32_t* table) {
  const uint32_t lo = crc_slice_begin(total, lanes, i), hi = crc_slice_begin(total, lanes, i + 1);
  uint32_t term = crc_shift(crc_run(0, out + lo, hi - lo, table), total - hi);
  if (i == 0) term ^= crc_shift(0xffffffffu, total);
  return term;
}

}  // namespace inflate
}  // namespace smh
