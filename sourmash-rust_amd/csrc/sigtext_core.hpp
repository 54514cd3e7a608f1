// sigtext_core.hpp -- the rules by which a resident index becomes signature JSON text (the rules are in
// include/sourmash_amd.h, "Signature JSON written on the device", and as plain Python in tests/sigtext_restatement.py), as one
// source for the device kernels (sigtext_kernels.hip) and for a plain host build (tests/c_sigtext_host.cpp): the digit count
// of a value, the formatter of one value, the MD5 block function with its padding, the layout arithmetic, and write_serial(),
// the serial driver that produces the whole text and every node's md5.  No HIP header is needed: the qualifiers sit behind
// SMH_HD and the unroll hints behind SMH_UNROLL.  Md5, the streaming form of the block function, is the library's one MD5 (signature.cpp's sketch_md5 uses it).
//
// Decimal digits.  A value is split at 10^9 and 10^18 into three 32-bit pieces (two 64-bit divisions by a compile-time
// constant, which the compiler turns into multiply-high; no division by a run-time value anywhere), and every piece is
// taken apart with 32-bit arithmetic.
#pragma once
#include <stdint.h>

#if !defined(SMH_HD)
#if defined(__HIPCC__)
#define SMH_HD __host__ __device__
#else
#define SMH_HD
#endif
#endif

// (a plain g++ knows no `#pragma unroll`)
#if defined(__clang__)
#define SMH_UNROLL _Pragma("unroll")
#else
#define SMH_UNROLL
#endif

#include <string.h>

#include <string>
#include <vector>

namespace smh {
namespace sigtext {

constexpr uint32_t kMaxDigits64 = 20, kMaxDigits32 = 10;
constexpr uint32_t kMd5InMid = 12;   // where the 32 hex digits stand in a node's middle piece: behind `],"md5sum":"`

SMH_HD inline uint32_t digits_below_1e9(uint32_t v) {   // 1 .. 9; v < 10^9
  return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u);
}

struct Parts { uint32_t hi, mid, lo; };   // v = hi * 10^18 + mid * 10^9 + lo; hi <= 18, mid and lo below 10^9

SMH_HD inline Parts split(uint64_t v) {
  const uint64_t q = v / 1000000000ull;
  Parts p;
  p.lo = (uint32_t)(v - q * 1000000000ull);
  p.hi = (uint32_t)(q / 1000000000ull);
  p.mid = (uint32_t)(q - (uint64_t)p.hi * 1000000000ull);
  return p;
}

SMH_HD inline uint32_t digits_of(const Parts& p) {
  if (p.hi) return 18u + (p.hi >= 10u ? 2u : 1u);
  if (p.mid) return 9u + digits_below_1e9(p.mid);
  return digits_below_1e9(p.lo);
}
SMH_HD inline uint32_t digits_u64(uint64_t v) { return digits_of(split(v)); }
SMH_HD inline uint32_t digits_u32(uint32_t v) { return v >= 1000000000u ? 10u : digits_below_1e9(v); }

// the low `count` digits of x into out[at - count, at), the lowest last; returns at - count
SMH_HD inline uint32_t put_digits(uint32_t x, uint32_t count, uint8_t* out, uint32_t at) {
  SMH_UNROLL
  for (uint32_t i = 0; i < 9; i++) {
    if (i < count) {
      const uint32_t q = x / 10u;
      out[--at] = (uint8_t)('0' + (x - q * 10u));
      x = q;
    }
  }
  return at;
}

// The decimal digits of v into out[0, n), n = digits_u64(v); returns n.
SMH_HD inline uint32_t format_u64(uint64_t v, uint8_t* out) {
  const Parts p = split(v);
  const uint32_t n = digits_of(p);
  uint32_t at = put_digits(p.lo, n < 9u ? n : 9u, out, n);
  if (n > 9u) at = put_digits(p.mid, n - 9u < 9u ? n - 9u : 9u, out, at);
  if (n > 18u) put_digits(p.hi, n - 18u, out, at);
  return n;
}
SMH_HD inline uint32_t format_u32(uint32_t v, uint8_t* out) {
  const uint32_t n = digits_u32(v);
  const uint32_t hi = v / 1000000000u;
  const uint32_t at = put_digits(v - hi * 1000000000u, n < 9u ? n : 9u, out, n);
  if (n > 9u) put_digits(hi, 1, out, at);
  return n;
}

// the bytes of a numeric array's inside: its digits and a comma between neighbours
SMH_HD inline uint64_t array_bytes(uint64_t digits, uint64_t count) { return digits + (count ? count - 1 : 0); }

// ---------------------------------------------------------------------------------------------------------------
// MD5 (RFC 1321).  M: the sixteen little-endian words of a block.

struct Md5State { uint32_t a, b, c, d; };

SMH_HD inline void md5_init(Md5State& s) { s.a = 0x67452301u; s.b = 0xefcdab89u; s.c = 0x98badcfeu; s.d = 0x10325476u; }

SMH_HD inline uint32_t md5_rol(uint32_t x, uint32_t n) { return (x << n) | (x >> (32u - n)); }

#define SMH_MD5_F(x, y, z) ((z) ^ ((x) & ((y) ^ (z))))
#define SMH_MD5_G(x, y, z) ((y) ^ ((z) & ((x) ^ (y))))
#define SMH_MD5_H(x, y, z) ((x) ^ (y) ^ (z))
#define SMH_MD5_I(x, y, z) ((y) ^ ((x) | ~(z)))
#define SMH_MD5_STEP(f, a, b, c, d, g, k, r) a = b + md5_rol(a + f(b, c, d) + M[g] + k, r)

SMH_HD inline void md5_block(Md5State& s, const uint32_t* M) {
  uint32_t a = s.a, b = s.b, c = s.c, d = s.d;
  SMH_MD5_STEP(SMH_MD5_F, a, b, c, d, 0, 0xd76aa478u, 7);   SMH_MD5_STEP(SMH_MD5_F, d, a, b, c, 1, 0xe8c7b756u, 12);
  SMH_MD5_STEP(SMH_MD5_F, c, d, a, b, 2, 0x242070dbu, 17);  SMH_MD5_STEP(SMH_MD5_F, b, c, d, a, 3, 0xc1bdceeeu, 22);
  SMH_MD5_STEP(SMH_MD5_F, a, b, c, d, 4, 0xf57c0fafu, 7);   SMH_MD5_STEP(SMH_MD5_F, d, a, b, c, 5, 0x4787c62au, 12);
  SMH_MD5_STEP(SMH_MD5_F, c, d, a, b, 6, 0xa8304613u, 17);  SMH_MD5_STEP(SMH_MD5_F, b, c, d, a, 7, 0xfd469501u, 22);
  SMH_MD5_STEP(SMH_MD5_F, a, b, c, d, 8, 0x698098d8u, 7);   SMH_MD5_STEP(SMH_MD5_F, d, a, b, c, 9, 0x8b44f7afu, 12);
  SMH_MD5_STEP(SMH_MD5_F, c, d, a, b, 10, 0xffff5bb1u, 17); SMH_MD5_STEP(SMH_MD5_F, b, c, d, a, 11, 0x895cd7beu, 22);
  SMH_MD5_STEP(SMH_MD5_F, a, b, c, d, 12, 0x6b901122u, 7);  SMH_MD5_STEP(SMH_MD5_F, d, a, b, c, 13, 0xfd987193u, 12);
  SMH_MD5_STEP(SMH_MD5_F, c, d, a, b, 14, 0xa679438eu, 17); SMH_MD5_STEP(SMH_MD5_F, b, c, d, a, 15, 0x49b40821u, 22);
  SMH_MD5_STEP(SMH_MD5_G, a, b, c, d, 1, 0xf61e2562u, 5);   SMH_MD5_STEP(SMH_MD5_G, d, a, b, c, 6, 0xc040b340u, 9);
  SMH_MD5_STEP(SMH_MD5_G, c, d, a, b, 11, 0x265e5a51u, 14); SMH_MD5_STEP(SMH_MD5_G, b, c, d, a, 0, 0xe9b6c7aau, 20);
  SMH_MD5_STEP(SMH_MD5_G, a, b, c, d, 5, 0xd62f105du, 5);   SMH_MD5_STEP(SMH_MD5_G, d, a, b, c, 10, 0x02441453u, 9);
  SMH_MD5_STEP(SMH_MD5_G, c, d, a, b, 15, 0xd8a1e681u, 14); SMH_MD5_STEP(SMH_MD5_G, b, c, d, a, 4, 0xe7d3fbc8u, 20);
  SMH_MD5_STEP(SMH_MD5_G, a, b, c, d, 9, 0x21e1cde6u, 5);   SMH_MD5_STEP(SMH_MD5_G, d, a, b, c, 14, 0xc33707d6u, 9);
  SMH_MD5_STEP(SMH_MD5_G, c, d, a, b, 3, 0xf4d50d87u, 14);  SMH_MD5_STEP(SMH_MD5_G, b, c, d, a, 8, 0x455a14edu, 20);
  SMH_MD5_STEP(SMH_MD5_G, a, b, c, d, 13, 0xa9e3e905u, 5);  SMH_MD5_STEP(SMH_MD5_G, d, a, b, c, 2, 0xfcefa3f8u, 9);
  SMH_MD5_STEP(SMH_MD5_G, c, d, a, b, 7, 0x676f02d9u, 14);  SMH_MD5_STEP(SMH_MD5_G, b, c, d, a, 12, 0x8d2a4c8au, 20);
  SMH_MD5_STEP(SMH_MD5_H, a, b, c, d, 5, 0xfffa3942u, 4);   SMH_MD5_STEP(SMH_MD5_H, d, a, b, c, 8, 0x8771f681u, 11);
  SMH_MD5_STEP(SMH_MD5_H, c, d, a, b, 11, 0x6d9d6122u, 16); SMH_MD5_STEP(SMH_MD5_H, b, c, d, a, 14, 0xfde5380cu, 23);
  SMH_MD5_STEP(SMH_MD5_H, a, b, c, d, 1, 0xa4beea44u, 4);   SMH_MD5_STEP(SMH_MD5_H, d, a, b, c, 4, 0x4bdecfa9u, 11);
  SMH_MD5_STEP(SMH_MD5_H, c, d, a, b, 7, 0xf6bb4b60u, 16);  SMH_MD5_STEP(SMH_MD5_H, b, c, d, a, 10, 0xbebfbc70u, 23);
  SMH_MD5_STEP(SMH_MD5_H, a, b, c, d, 13, 0x289b7ec6u, 4);  SMH_MD5_STEP(SMH_MD5_H, d, a, b, c, 0, 0xeaa127fau, 11);
  SMH_MD5_STEP(SMH_MD5_H, c, d, a, b, 3, 0xd4ef3085u, 16);  SMH_MD5_STEP(SMH_MD5_H, b, c, d, a, 6, 0x04881d05u, 23);
  SMH_MD5_STEP(SMH_MD5_H, a, b, c, d, 9, 0xd9d4d039u, 4);   SMH_MD5_STEP(SMH_MD5_H, d, a, b, c, 12, 0xe6db99e5u, 11);
  SMH_MD5_STEP(SMH_MD5_H, c, d, a, b, 15, 0x1fa27cf8u, 16); SMH_MD5_STEP(SMH_MD5_H, b, c, d, a, 2, 0xc4ac5665u, 23);
  SMH_MD5_STEP(SMH_MD5_I, a, b, c, d, 0, 0xf4292244u, 6);   SMH_MD5_STEP(SMH_MD5_I, d, a, b, c, 7, 0x432aff97u, 10);
  SMH_MD5_STEP(SMH_MD5_I, c, d, a, b, 14, 0xab9423a7u, 15); SMH_MD5_STEP(SMH_MD5_I, b, c, d, a, 5, 0xfc93a039u, 21);
  SMH_MD5_STEP(SMH_MD5_I, a, b, c, d, 12, 0x655b59c3u, 6);  SMH_MD5_STEP(SMH_MD5_I, d, a, b, c, 3, 0x8f0ccc92u, 10);
  SMH_MD5_STEP(SMH_MD5_I, c, d, a, b, 10, 0xffeff47du, 15); SMH_MD5_STEP(SMH_MD5_I, b, c, d, a, 1, 0x85845dd1u, 21);
  SMH_MD5_STEP(SMH_MD5_I, a, b, c, d, 8, 0x6fa87e4fu, 6);   SMH_MD5_STEP(SMH_MD5_I, d, a, b, c, 15, 0xfe2ce6e0u, 10);
  SMH_MD5_STEP(SMH_MD5_I, c, d, a, b, 6, 0xa3014314u, 15);  SMH_MD5_STEP(SMH_MD5_I, b, c, d, a, 13, 0x4e0811a1u, 21);
  SMH_MD5_STEP(SMH_MD5_I, a, b, c, d, 4, 0xf7537e82u, 6);   SMH_MD5_STEP(SMH_MD5_I, d, a, b, c, 11, 0xbd3af235u, 10);
  SMH_MD5_STEP(SMH_MD5_I, c, d, a, b, 2, 0x2ad7d2bbu, 15);  SMH_MD5_STEP(SMH_MD5_I, b, c, d, a, 9, 0xeb86d391u, 21);
  s.a += a; s.b += b; s.c += c; s.d += d;
}

#undef SMH_MD5_STEP
#undef SMH_MD5_I
#undef SMH_MD5_H
#undef SMH_MD5_G
#undef SMH_MD5_F

// RFC 1321's padding as words.  The message's last `fill` bytes (fill < 64) stand in tail[0, fill) of a buffer of 32 words
// that the caller may read as bytes; pad_word(w, ...) is word w of the one or two closing blocks (md5_pad_blocks of them):
// the tail's own bytes, 0x80, zeros, and the length in bits in the last two words.  Bytes of the buffer at or behind `fill`
// are not read.
SMH_HD inline uint32_t md5_pad_blocks(uint32_t fill) { return fill < 56u ? 1u : 2u; }
SMH_HD inline uint32_t md5_pad_word(const uint8_t* tail, uint32_t fill, uint64_t total_bytes, uint32_t w) {
  const uint32_t last = md5_pad_blocks(fill) * 16u - 2u;
  if (w == last) return (uint32_t)(total_bytes << 3);
  if (w == last + 1u) return (uint32_t)(total_bytes >> 29);
  uint32_t x = 0;
  SMH_UNROLL
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t at = 4u * w + k;
    const uint32_t byte = at < fill ? (uint32_t)tail[at] : at == fill ? 0x80u : 0u;
    x |= byte << (8u * k);
  }
  return x;
}
// closes the chain: s becomes the digest's four words
SMH_HD inline void md5_finish(Md5State& s, const uint8_t* tail, uint32_t fill, uint64_t total_bytes) {
  const uint32_t nb = md5_pad_blocks(fill);
  for (uint32_t b = 0; b < nb; b++) {
    uint32_t M[16];
  SMH_UNROLL
    for (uint32_t w = 0; w < 16; w++) M[w] = md5_pad_word(tail, fill, total_bytes, b * 16u + w);
    md5_block(s, M);
  }
}
// byte i (0 .. 15) of the digest
SMH_HD inline uint32_t md5_digest_byte(const Md5State& s, uint32_t i) {
  const uint32_t w = i < 4 ? s.a : i < 8 ? s.b : i < 12 ? s.c : s.d;
  return (w >> (8u * (i & 3u))) & 0xffu;
}
SMH_HD inline uint8_t hex_digit(uint32_t v) { return (uint8_t)(v < 10u ? '0' + v : 'a' + (v - 10u)); }

// ---------------------------------------------------------------------------------------------------------------
// host only from here (plain functions: a HIP compile sees them in both of its passes and emits them for the host alone)

#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "Md5 copies message bytes into words: a little-endian host is assumed"
#endif

// the streaming form
struct Md5 {
  Md5State st;
  uint64_t total = 0;
  uint32_t words[16];
  uint32_t fill = 0;
  Md5() { md5_init(st); }
  void update(const void* data, size_t n) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    total += n;
    while (n) {
      const size_t take = n < (size_t)(64u - fill) ? n : (size_t)(64u - fill);
      memcpy(reinterpret_cast<uint8_t*>(words) + fill, p, take);
      fill += (uint32_t)take; p += take; n -= take;
      if (fill == 64) { md5_block(st, words); fill = 0; }
    }
  }
  void digest(uint8_t* out16) {   // closes the chain: call once
    md5_finish(st, reinterpret_cast<const uint8_t*>(words), fill, total);
    for (uint32_t i = 0; i < 16; i++) out16[i] = (uint8_t)md5_digest_byte(st, i);
  }
  std::string hex() {
    uint8_t d[16];
    digest(d);
    std::string out(32, '0');
    for (uint32_t i = 0; i < 16; i++) { out[2 * i] = (char)hex_digit(d[i] >> 4); out[2 * i + 1] = (char)hex_digit(d[i] & 15u); }
    return out;
  }
};

// What the host knows of a node: the three pieces of its signature around the two arrays.
//   head   {"class": ... up to and including "mins":[
//   mid    ],"md5sum":" + 32 placeholder bytes + " and, with abundances, ,"abundances":[
//   tail   the rest: (] with abundances) ,"molecule":"..."}],"version":0.4}
struct NodeText { std::string head, mid, tail; };
struct NodeParams { uint32_t num, ksize; uint64_t seed, max_hash; const char* molecule; };

// filename_json / name_json: the JSON value as it stands in the text -- `null`, or the string escaped and quoted
inline NodeText node_text(const NodeParams& p, const std::string& filename_json, const std::string& name_json, bool has_abunds) {
  NodeText t;
  t.head = "{\"class\":\"sourmash_signature\",\"email\":\"\",\"hash_function\":\"0.murmur64\",\"filename\":" + filename_json + ",\"name\":" + name_json +
           ",\"license\":\"CC0\",\"signatures\":[{\"num\":" + std::to_string(p.num) + ",\"ksize\":" + std::to_string(p.ksize) + ",\"seed\":" +
           std::to_string(p.seed) + ",\"max_hash\":" + std::to_string(p.max_hash) + ",\"mins\":[";
  t.mid = "],\"md5sum\":\"" + std::string(32, '0') + "\"";
  if (has_abunds) t.mid += ",\"abundances\":[";
  t.tail = std::string(has_abunds ? "]" : "") + ",\"molecule\":\"" + p.molecule + "\"}],\"version\":0.4}";
  return t;
}

// The layout walk, the one place that says where everything stands.  Document d holds the nodes [doc_starts[d], doc_starts[d + 1])
// (doc_starts null: one document of all n nodes).  hash_digits[v] / abund_digits[v]: the digit totals of node v's arrays,
// counts[v] its values.  The sink is told, in text order:
//   sink.document(d, at)                     document d begins at `at`
//   sink.piece(bytes, len, at)               skeleton bytes
//   sink.mins(v, at) / sink.abunds(v, at)    where the inside of node v's array begins
//   sink.md5(v, at)                          where node v's 32 hex digits stand
// Returns the length of the text.
template <class Sink>
inline uint64_t walk_layout(uint32_t n, const uint32_t* doc_starts, uint32_t n_docs, const NodeText* nodes, const uint64_t* hash_digits,
                            const uint64_t* abund_digits, const uint64_t* counts, bool has_abunds, Sink& sink) {
  const uint32_t whole[2] = {0, n};
  if (!doc_starts) { doc_starts = whole; n_docs = 1; }
  uint64_t at = 0;
  for (uint32_t d = 0; d < n_docs; d++) {
    sink.document(d, at);
    sink.piece("[", 1, at); at += 1;
    for (uint32_t v = doc_starts[d]; v < doc_starts[d + 1]; v++) {
      const NodeText& t = nodes[v];
      if (v != doc_starts[d]) { sink.piece(",", 1, at); at += 1; }
      sink.piece(t.head.data(), t.head.size(), at); at += t.head.size();
      sink.mins(v, at); at += array_bytes(hash_digits[v], counts[v]);
      sink.piece(t.mid.data(), t.mid.size(), at);
      sink.md5(v, at + kMd5InMid); at += t.mid.size();   // (behind the piece: the digits replace its placeholder)
      if (has_abunds) { sink.abunds(v, at); at += array_bytes(abund_digits[v], counts[v]); }
      sink.piece(t.tail.data(), t.tail.size(), at); at += t.tail.size();
    }
    sink.piece("]", 1, at); at += 1;
  }
  sink.document(n_docs, at);
  return at;
}

// The serial driver: the whole text, where its documents begin (n_docs + 1 entries) and every node's md5 (16 n bytes).
// offsets: n + 1, from 0; abunds null: an index without abundances.
struct SerialSink {
  std::string* text;
  std::vector<uint64_t>* doc_offsets;
  std::vector<uint8_t>* digests;
  const uint64_t *offsets, *hashes;
  const uint32_t* abund_values;
  void at_least(uint64_t end) { if (text->size() < end) text->resize(end); }
  void document(uint32_t d, uint64_t at) { if (doc_offsets->size() <= d) doc_offsets->resize((size_t)d + 1); (*doc_offsets)[d] = at; }
  void piece(const char* bytes, uint64_t len, uint64_t at) { at_least(at + len); memcpy(&(*text)[at], bytes, len); }
  template <class V, class F> void array(const V* values, uint64_t count, uint64_t at, F format) {
    uint8_t tmp[kMaxDigits64];
    for (uint64_t i = 0; i < count; i++) {
      if (i) { at_least(at + 1); (*text)[at++] = ','; }
      const uint32_t k = format(values[i], tmp);
      at_least(at + k); memcpy(&(*text)[at], tmp, k); at += k;
    }
  }
  void mins(uint32_t v, uint64_t at) { array(hashes + offsets[v], offsets[v + 1] - offsets[v], at, format_u64); }
  void abunds(uint32_t v, uint64_t at) { array(abund_values + offsets[v], offsets[v + 1] - offsets[v], at, format_u32); }
  void md5(uint32_t v, uint64_t at) {
    at_least(at + 32);
    for (uint32_t i = 0; i < 16; i++) {
      const uint8_t b = (*digests)[(size_t)v * 16 + i];
      (*text)[at + 2 * i] = (char)hex_digit(b >> 4); (*text)[at + 2 * i + 1] = (char)hex_digit(b & 15u);
    }
  }
};

// the md5 of str(ksize) followed by the decimal hashes, no separator
inline void node_md5(uint32_t ksize, const uint64_t* hashes, uint64_t count, uint8_t* out16) {
  Md5 m;
  uint8_t tmp[kMaxDigits64];
  m.update(tmp, format_u32(ksize, tmp));
  for (uint64_t i = 0; i < count; i++) m.update(tmp, format_u64(hashes[i], tmp));
  m.digest(out16);
}

inline void write_serial(uint32_t n, const uint64_t* offsets, const uint64_t* hashes, const uint32_t* abunds, const uint32_t* ksizes,
                         const NodeText* nodes, const uint32_t* doc_starts, uint32_t n_docs, std::string* text,
                         std::vector<uint64_t>* doc_offsets, std::vector<uint8_t>* md5) {
  std::vector<uint64_t> hd(n, 0), ad(n, 0), counts(n, 0);
  md5->assign((size_t)n * 16, 0);
  for (uint32_t v = 0; v < n; v++) {
    counts[v] = offsets[v + 1] - offsets[v];
    for (uint64_t i = offsets[v]; i < offsets[v + 1]; i++) {
      hd[v] += digits_u64(hashes[i]);
      if (abunds) ad[v] += digits_u32(abunds[i]);
    }
    node_md5(ksizes[v], hashes + offsets[v], counts[v], md5->data() + (size_t)v * 16);
  }
  text->clear();
  doc_offsets->clear();
  SerialSink sink{text, doc_offsets, md5, offsets, hashes, abunds};
  const uint64_t len = walk_layout(n, doc_starts, n_docs, nodes, hd.data(), ad.data(), counts.data(), abunds != nullptr, sink);
  text->resize(len);
}

}  // namespace sigtext
}  // namespace smh
