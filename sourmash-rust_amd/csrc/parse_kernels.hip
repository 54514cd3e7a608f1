// parse_kernels.hip -- FASTA / FASTQ text resident in HBM -> the record layout of the sketching paths (one dense
// buffer of sequence bytes + offsets[n + 1]) and the records' name spans.  DESIGN.md 3.8.
//
// Three passes, no host work per record or per line:
//   1. k_parse_summary   one workgroup per tile of kParseTileBytes: what the tile contributes, as a function of the
//                        state it is entered in (an element of the scan's monoid);
//   2. k_scan_*          an ordered scan of the tile elements with 64-bit positions: the entering state of every tile
//                        (class of the running line / line number, output position, record index) and the totals;
//   3. k_parse_compact   the same classification again, now with the entering state: kept bytes go through LDS to the
//                        dense buffer in whole 16-byte segments, record starts write offsets and name spans, the
//                        format checks lower an error word with atomicMin.
// Tiles are cut on 16-byte boundaries of the ADDRESS, so every full chunk is one aligned 16-byte load whatever the
// alignment of the text pointer; the chunks that hold the text's first and last bytes are read byte by byte and
// nothing outside [text, text + len) is touched.
#include "kernels.hpp"

namespace smh {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTile = kParseTileBytes;
static_assert(kTile == kThreads * 16, "one 16-byte chunk per thread");

enum : uint32_t { kClsNone = 0, kClsSeq = 1, kClsHdr = 2 };

// ---------------------------------------------------------------------------------------------------------------
// one thread's 16 bytes

struct Chunk {
  uint64_t lo, hi;     // bytes 0..7, 8..15 (0 where not valid)
  uint32_t valid;      // bit j: byte j is a byte of the text
  int64_t pos0;        // text position of byte 0 (negative in the chunk that holds the text's first byte)
};

__device__ __forceinline__ uint32_t byte_of(const Chunk& c, uint32_t j) {
  return (uint32_t)(((j < 8 ? c.lo : c.hi) >> ((j & 7) * 8)) & 0xff);
}

__device__ __forceinline__ Chunk load_chunk(const uint8_t* abase, uint32_t lead, uint64_t len, uint64_t tile, uint32_t tid) {
  Chunk c;
  const uint64_t ai = tile * kTile + (uint64_t)tid * 16;
  c.pos0 = (int64_t)ai - (int64_t)lead;
  if (c.pos0 >= 0 && (uint64_t)c.pos0 + 16 <= len) {
    const uint4 v = *reinterpret_cast<const uint4*>(abase + ai);
    c.lo = (uint64_t)v.x | ((uint64_t)v.y << 32);
    c.hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
    c.valid = 0xffffu;
  } else {
    c.lo = c.hi = 0; c.valid = 0;
    for (uint32_t j = 0; j < 16; j++) {
      const int64_t p = c.pos0 + j;
      if (p >= 0 && (uint64_t)p < len) {
        const uint64_t b = abase[ai + j];
        if (j < 8) c.lo |= b << (j * 8); else c.hi |= b << ((j - 8) * 8);
        c.valid |= 1u << j;
      }
    }
  }
  return c;
}

// bit i of the result: byte i of w equals ch
__device__ __forceinline__ uint32_t eq4(uint32_t w, uint32_t ch) {
  const uint32_t x = w ^ (ch * 0x01010101u);
  const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);   // 0x80 in every zero byte of x
  return ((t >> 7) * 0x01020408u) >> 24;
}
__device__ __forceinline__ uint32_t eq16(const Chunk& c, uint32_t ch) {
  return eq4((uint32_t)c.lo, ch) | (eq4((uint32_t)(c.lo >> 32), ch) << 4) | (eq4((uint32_t)c.hi, ch) << 8) |
         (eq4((uint32_t)(c.hi >> 32), ch) << 12);
}

// The line structure of a chunk, by the rules of the format contract: a line ends at '\n'; one '\r' directly in front of
// it, or a '\r' that is the text's last byte, belongs to the terminator; everything else is content.
struct Lines {
  uint32_t nl;        // '\n'
  uint32_t content;   // bytes that are not part of a terminator
  uint32_t ls;        // line starts
  uint32_t ends;      // where a line ends: its '\n', or the text's last byte when that is no '\n'
  uint32_t cr_before; // bit j: the byte in front of byte j is '\r'
};

__device__ __forceinline__ Lines classify(const Chunk& c, uint64_t len, const uint8_t* text, uint8_t* sh_first, uint8_t* sh_last,
                                          uint32_t tid) {
  // neighbours: the byte in front of the chunk and the byte behind it, through LDS inside the tile
  sh_first[tid] = (uint8_t)(c.lo & 0xff);
  sh_last[tid] = (uint8_t)(c.hi >> 56);
  __syncthreads();
  uint32_t prevb = 0, nextb = 0;
  if (tid > 0) prevb = sh_last[tid - 1];
  else if (c.pos0 > 0) prevb = text[c.pos0 - 1];
  if (tid + 1 < kThreads) nextb = sh_first[tid + 1];
  else if (c.pos0 + 16 >= 0 && (uint64_t)(c.pos0 + 16) < len) nextb = text[c.pos0 + 16];
  Lines L;
  L.nl = eq16(c, '\n') & c.valid;
  const uint32_t cr = eq16(c, '\r') & c.valid;
  const int64_t jl = (int64_t)len - 1 - c.pos0;                 // where the text's last byte is
  const uint32_t lastbit = (jl >= 0 && jl < 16) ? 1u << jl : 0u;
  const uint32_t term = L.nl | (cr & ((L.nl >> 1) | (nextb == '\n' ? 0x8000u : 0u) | lastbit));
  L.content = c.valid & ~term;
  L.ls = ((L.nl << 1) | (c.pos0 > 0 && prevb == '\n' ? 1u : 0u)) & c.valid;
  if (c.pos0 <= 0 && c.pos0 > -16) L.ls |= (1u << (uint32_t)(-c.pos0)) & c.valid;   // position 0 starts a line
  L.ends = L.nl | (lastbit & ~L.nl & c.valid);
  L.cr_before = ((cr << 1) | (prevb == '\r' ? 1u : 0u)) & 0xffffu;
  return L;
}

__device__ __forceinline__ uint32_t below(uint32_t j) { return (1u << j) - 1u; }

// ---------------------------------------------------------------------------------------------------------------
// workgroup primitives (256 threads = 4 waves)

// exclusive prefix sum of v over the workgroup; *total = the sum.  sh: 4 words.
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* total, uint32_t* sh, uint32_t tid) {
  const uint32_t lane = tid & 63, wave = tid >> 6;
  uint32_t inc = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();            // sh may still be read from an earlier call
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kThreads / 64; w++) {
    const uint32_t s = sh[w];
    if (w < wave) base += s;
    all += s;
  }
  *total = all;
  return base + inc - v;
}

// FASTA: the class of the line that runs into this thread's chunk = the class of the nearest earlier line start of the
// tile, else tile_cls.  has = this chunk holds a line start, last_hdr = its last one starts a header.  sh: 8 qwords.
// *tile_last = the class of the last line start of the tile (kClsNone: the tile holds none).
__device__ __forceinline__ uint32_t block_enter_class(bool has, bool last_hdr, uint32_t tile_cls, uint32_t* tile_last,
                                                      uint64_t* sh, uint32_t tid) {
  const uint32_t lane = tid & 63, wave = tid >> 6;
  const uint64_t bh = __ballot(has), bl = __ballot(last_hdr);
  __syncthreads();
  if (lane == 0) { sh[wave] = bh; sh[4 + wave] = bl; }
  __syncthreads();
  uint32_t cls = kClsNone, last = kClsNone;
  const uint64_t mine = bh & ((1ull << lane) - 1ull);
  if (mine) cls = ((bl >> (63 - __clzll((long long)mine))) & 1) ? kClsHdr : kClsSeq;
#pragma unroll
  for (int w = kThreads / 64 - 1; w >= 0; w--) {
    const uint64_t h = sh[w];
    if (!h) continue;
    const uint32_t k = ((sh[4 + w] >> (63 - __clzll((long long)h))) & 1) ? kClsHdr : kClsSeq;
    if (last == kClsNone) last = k;
    if (cls == kClsNone && w < (int)wave) cls = k;
  }
  *tile_last = last;
  return cls == kClsNone ? tile_cls : cls;
}

// FASTA: hdr = the line starts that hold '>', in_hdr = the bytes that lie on a header line, given whether the line that
// runs into the chunk is one.  A header's bit is carried up to the next line start by one addition.
__device__ __forceinline__ uint32_t header_starts(const Chunk& c, uint32_t ls) {
  uint32_t hdr = 0;
  for (uint32_t m = ls; m; m &= m - 1) {
    const uint32_t j = __builtin_ctz(m);
    if (byte_of(c, j) == '>') hdr |= 1u << j;
  }
  return hdr;
}
__device__ __forceinline__ uint32_t header_bytes(uint32_t ls, uint32_t hdr, bool enter_hdr) {
  const uint32_t LS = (ls << 1) | 1u;                 // bit 0: the line that runs in
  const uint32_t H = (hdr << 1) | (enter_hdr ? 1u : 0u);
  const uint32_t P = ~LS & 0x1ffffu;
  const uint32_t sum = (H << 1) + P;
  return ((H | ((sum ^ P) & P)) >> 1) & 0xffffu;
}

// FASTQ: the content bytes that lie on lines whose number is 1 and 3 mod 4, given the number of the line that holds
// byte 0 of the chunk.
__device__ __forceinline__ void fastq_roles(uint32_t nl, uint32_t content, uint32_t line0, uint32_t* seqm, uint32_t* qualm) {
  uint32_t s = 0, q = 0, rem = 0xffffu, nm = nl, cur = line0 & 3;
  while (true) {
    const uint32_t seg = (nm ? (((nm & (0u - nm)) << 1) - 1u) : 0xffffu) & rem;   // up to and including the next '\n'
    if (cur == 1) s |= seg;
    if (cur == 3) q |= seg;
    rem &= ~seg;
    if (!nm) break;
    nm &= nm - 1;
    cur = (cur + 1) & 3;
  }
  *seqm = s & content;
  *qualm = q & content;
}

// ---------------------------------------------------------------------------------------------------------------
// pass 1: tile summaries (16 bytes per tile)

struct TileSum { uint32_t a, b, c, d; };
// FASTA: a = class of the tile's last line start, b = content bytes in front of its first line start (kept when the
//        tile is entered on a sequence line), c = kept bytes behind it, d = record starts.
// FASTQ: a = '\n' bytes, b = 1 + the '\n' bytes in front of the tile's last content byte (0: no content),
//        c | d << 32 = content bytes by (line number inside the tile) mod 4, 16 bits each.

__global__ __launch_bounds__(kThreads) void k_parse_summary_fasta(const uint8_t* text, uint32_t lead, uint64_t len, TileSum* sums) {
  __shared__ uint8_t sh_first[kThreads], sh_last[kThreads];
  __shared__ uint64_t sh64[8];
  __shared__ uint32_t sh32[4];
  const uint32_t tid = threadIdx.x;
  const uint64_t tile = blockIdx.x;
  const Chunk c = load_chunk(text - lead, lead, len, tile, tid);
  const Lines L = classify(c, len, text, sh_first, sh_last, tid);
  const uint32_t hdr = header_starts(c, L.ls);
  const bool has = L.ls != 0;
  const bool last_hdr = has && ((hdr >> (31 - __builtin_clz(L.ls))) & 1);
  uint32_t tile_last;
  const uint32_t enter = block_enter_class(has, last_hdr, kClsNone, &tile_last, sh64, tid);
  const uint32_t kept = L.content & ~header_bytes(L.ls, hdr, enter == kClsHdr);
  uint32_t pre = 0, post = __builtin_popcount(kept);
  if (enter == kClsNone) {
    const uint32_t front = has ? below(__builtin_ctz(L.ls)) : 0xffffu;
    pre = __builtin_popcount(L.content & front);
    post = __builtin_popcount(kept & ~front);
  }
  uint32_t t_cnt, t_hdr;
  block_scan_excl(pre | (post << 16), &t_cnt, sh32, tid);     // each at most 4096
  block_scan_excl(__builtin_popcount(hdr), &t_hdr, sh32, tid);
  if (tid == 0) sums[tile] = TileSum{tile_last, t_cnt & 0xffffu, t_cnt >> 16, t_hdr};
}

__global__ __launch_bounds__(kThreads) void k_parse_summary_fastq(const uint8_t* text, uint32_t lead, uint64_t len, TileSum* sums) {
  __shared__ uint8_t sh_first[kThreads], sh_last[kThreads];
  __shared__ uint32_t sh32[4];
  __shared__ uint32_t sh_max;
  const uint32_t tid = threadIdx.x;
  const uint64_t tile = blockIdx.x;
  if (tid == 0) sh_max = 0;
  const Chunk c = load_chunk(text - lead, lead, len, tile, tid);
  const Lines L = classify(c, len, text, sh_first, sh_last, tid);
  uint32_t t_nl;
  const uint32_t nl0 = block_scan_excl(__builtin_popcount(L.nl), &t_nl, sh32, tid);
  // content bytes by line number inside the tile, mod 4: four passes of 16-bit sums (a tile holds at most 4096 bytes)
  uint32_t cnt[4] = {0, 0, 0, 0};
  {
    uint32_t rem = 0xffffu, nm = L.nl, cur = nl0 & 3;
    while (true) {
      const uint32_t seg = (nm ? (((nm & (0u - nm)) << 1) - 1u) : 0xffffu) & rem;
      const uint32_t k = __builtin_popcount(seg & L.content);
      cnt[0] += cur == 0 ? k : 0; cnt[1] += cur == 1 ? k : 0; cnt[2] += cur == 2 ? k : 0; cnt[3] += cur == 3 ? k : 0;
      rem &= ~seg;
      if (!nm) break;
      nm &= nm - 1;
      cur = (cur + 1) & 3;
    }
  }
  uint32_t t01, t23;
  block_scan_excl(cnt[0] | (cnt[1] << 16), &t01, sh32, tid);   // a field reaches 4096 at most: no carry into its neighbour
  block_scan_excl(cnt[2] | (cnt[3] << 16), &t23, sh32, tid);
  if (L.content) {
    const uint32_t j = 31 - __builtin_clz(L.content);
    atomicMax(&sh_max, nl0 + __builtin_popcount(L.nl & below(j)) + 1);
  }
  __syncthreads();
  if (tid == 0) sums[tile] = TileSum{t_nl, sh_max, t01, t23};
}

// ---------------------------------------------------------------------------------------------------------------
// pass 2: the ordered scan over the tiles, 64-bit throughout.  Each format brings the monoid: Elem, identity(), load(),
// combine(earlier, later), the state a tile is entered in given the caller's first state and the product of the tiles in
// front of it, and the totals.

struct FastaScan {
  struct Elem { uint64_t pre, post, nhdr; uint32_t cls; };
  static __device__ Elem identity() { return Elem{0, 0, 0, kClsNone}; }
  static __device__ Elem load(const TileSum& t) { return Elem{t.b, t.c, t.d, t.a}; }
  // a tile (or run of tiles) is a function of the class it is entered in: kept = (class == sequence ? pre : 0) + post
  static __device__ Elem combine(const Elem& x, const Elem& y) {
    Elem r;
    r.nhdr = x.nhdr + y.nhdr;
    r.cls = y.cls != kClsNone ? y.cls : x.cls;
    if (x.cls == kClsNone) { r.pre = x.pre + y.pre; r.post = y.post; }        // x holds no line start: x.post == 0
    else { r.pre = x.pre; r.post = x.post + (x.cls == kClsSeq ? y.pre : 0) + y.post; }
    return r;
  }
  static __device__ ParseTileIn state(const ParseTileIn& first, const Elem& p) {
    ParseTileIn s;
    s.outpos = first.outpos + (first.cls == kClsSeq ? p.pre : 0) + p.post;
    s.count = first.count + p.nhdr;
    s.bal = 0;
    s.cls = p.cls != kClsNone ? p.cls : first.cls;
    s.pad = 0;
    return s;
  }
  static __device__ void totals(const ParseTileIn& first, const Elem& p, ParseTotals* out) {
    const ParseTileIn s = state(first, p);
    out->n_records = s.count; out->total = s.outpos; out->lines = 0; out->balance = 0; out->err = ~0ull;
  }
};

struct FastqScan {
  struct Elem { uint64_t nl, lines, c[4]; };
  static __device__ Elem identity() { return Elem{0, 0, {0, 0, 0, 0}}; }
  static __device__ Elem load(const TileSum& t) {
    return Elem{t.a, t.b, {t.c & 0xffffu, t.c >> 16, t.d & 0xffffu, t.d >> 16}};
  }
  // c[j] counts the content bytes on the lines numbered j mod 4 from the run's first line: the later run's counts are
  // rotated by the earlier run's line count.  lines = 1 + the number of the last line that has content (0: none).
  static __device__ Elem combine(const Elem& x, const Elem& y) {
    Elem r;
    r.nl = x.nl + y.nl;
    r.lines = y.lines ? x.nl + y.lines : x.lines;
    switch (x.nl & 3) {
      case 0: r.c[0] = x.c[0] + y.c[0]; r.c[1] = x.c[1] + y.c[1]; r.c[2] = x.c[2] + y.c[2]; r.c[3] = x.c[3] + y.c[3]; break;
      case 1: r.c[0] = x.c[0] + y.c[3]; r.c[1] = x.c[1] + y.c[0]; r.c[2] = x.c[2] + y.c[1]; r.c[3] = x.c[3] + y.c[2]; break;
      case 2: r.c[0] = x.c[0] + y.c[2]; r.c[1] = x.c[1] + y.c[3]; r.c[2] = x.c[2] + y.c[0]; r.c[3] = x.c[3] + y.c[1]; break;
      default: r.c[0] = x.c[0] + y.c[1]; r.c[1] = x.c[1] + y.c[2]; r.c[2] = x.c[2] + y.c[3]; r.c[3] = x.c[3] + y.c[0]; break;
    }
    return r;
  }
  static __device__ void seq_qual(const ParseTileIn& first, const Elem& p, uint64_t* seq, uint64_t* qual) {
    switch (first.count & 3) {       // the caller's first line number decides which relative lines are sequence lines
      case 0: *seq = p.c[1]; *qual = p.c[3]; break;
      case 1: *seq = p.c[0]; *qual = p.c[2]; break;
      case 2: *seq = p.c[3]; *qual = p.c[1]; break;
      default: *seq = p.c[2]; *qual = p.c[0]; break;
    }
  }
  static __device__ ParseTileIn state(const ParseTileIn& first, const Elem& p) {
    uint64_t seq, qual;
    seq_qual(first, p, &seq, &qual);
    ParseTileIn s;
    s.outpos = first.outpos + seq;
    s.count = first.count + p.nl;
    s.bal = first.bal + (int64_t)seq - (int64_t)qual;
    s.cls = kClsNone; s.pad = 0;
    return s;
  }
  // After the empty lines at the end are dropped the text has `lines` lines.  A record cut short is malformed; one of
  // three lines is complete when its sequence line is empty -- every earlier record being sound, that is balance == 0.
  static __device__ void totals(const ParseTileIn& first, const Elem& p, ParseTotals* out) {
    const ParseTileIn s = state(first, p);
    const uint64_t lines = p.lines ? first.count + p.lines : 0;
    out->lines = lines;
    out->n_records = (lines + 3) / 4;
    out->total = s.outpos;
    out->balance = s.bal;
    const uint32_t part = (uint32_t)(lines & 3);
    out->err = (part == 1 || part == 2 || (part == 3 && s.bal != 0)) ? lines / 4 : ~0ull;
  }
};

// inclusive scan of one element per thread in LDS (order kept); returns this thread's inclusive value
template <class S>
__device__ __forceinline__ typename S::Elem block_scan_elems(typename S::Elem v, typename S::Elem* sh, uint32_t tid) {
  sh[tid] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kThreads; d <<= 1) {
    typename S::Elem o = v;
    if (tid >= d) o = S::combine(sh[tid - d], v);
    __syncthreads();
    v = o;
    sh[tid] = v;
    __syncthreads();
  }
  return v;
}

template <class S>
__global__ __launch_bounds__(kThreads) void k_scan_reduce(const TileSum* sums, uint64_t ntiles, typename S::Elem* agg) {
  __shared__ typename S::Elem sh[kThreads];
  const uint32_t tid = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + tid;
  block_scan_elems<S>(i < ntiles ? S::load(sums[i]) : S::identity(), sh, tid);
  if (tid == 0) agg[blockIdx.x] = sh[kThreads - 1];
}

// one workgroup: agg[b] -> the product of the blocks in front of b; the totals of the whole text
template <class S>
__global__ __launch_bounds__(kThreads) void k_scan_top(typename S::Elem* agg, uint64_t nblocks, ParseTileIn first, ParseTotals* totals) {
  __shared__ typename S::Elem sh[kThreads];
  const uint32_t tid = threadIdx.x;
  typename S::Elem carry = S::identity();
  for (uint64_t base = 0; base < nblocks; base += kThreads) {
    const uint64_t i = base + tid;
    block_scan_elems<S>(i < nblocks ? agg[i] : S::identity(), sh, tid);
    const typename S::Elem excl = tid ? S::combine(carry, sh[tid - 1]) : carry;
    const typename S::Elem next = S::combine(carry, sh[kThreads - 1]);
    __syncthreads();
    if (i < nblocks) agg[i] = excl;
    carry = next;
  }
  if (tid == 0) S::totals(first, carry, totals);
}

template <class S>
__global__ __launch_bounds__(kThreads) void k_scan_down(const TileSum* sums, uint64_t ntiles, const typename S::Elem* agg, ParseTileIn first,
                                                        ParseTileIn* states) {
  __shared__ typename S::Elem sh[kThreads];
  const uint32_t tid = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + tid;
  block_scan_elems<S>(i < ntiles ? S::load(sums[i]) : S::identity(), sh, tid);
  const typename S::Elem front = agg[blockIdx.x];
  if (i < ntiles) states[i] = S::state(first, tid ? S::combine(front, sh[tid - 1]) : front);
}

// ---------------------------------------------------------------------------------------------------------------
// pass 3: compaction

struct CompactArgs {
  const uint8_t* text; uint32_t lead; uint64_t len;
  const ParseTileIn* states;
  uint8_t* out;            // 16-byte aligned, room for total bytes
  uint64_t* offsets;       // n entries written here (offsets[n] = total is the host's)
  uint64_t* name_start;    // n
  uint64_t* name_end;      // n
  uint64_t n, total, lines;
  unsigned long long* err;
};

// kept bytes of the tile -> out[outpos .. outpos + K): staged in LDS at the output's own phase mod 16, so that every
// full 16-byte segment of the output is one aligned LDS read and one aligned store
__device__ __forceinline__ void stage_and_store(const Chunk& c, uint32_t kept, uint32_t kbase, uint32_t K, uint64_t outpos,
                                                const CompactArgs& a, uint8_t* stage, uint32_t tid) {
  const uint32_t shift = (uint32_t)(outpos & 15);
  uint32_t at = shift + kbase;
  if (kept == 0xffffu && (at & 3) == 0) {          // a whole chunk of sequence at a word boundary
    uint32_t* w = reinterpret_cast<uint32_t*>(stage + at);
    w[0] = (uint32_t)c.lo; w[1] = (uint32_t)(c.lo >> 32); w[2] = (uint32_t)c.hi; w[3] = (uint32_t)(c.hi >> 32);
  } else {
    for (uint32_t m = kept; m; m &= m - 1) stage[at++] = (uint8_t)byte_of(c, __builtin_ctz(m));
  }
  __syncthreads();
  if (outpos + K > a.total) return;                // cannot happen: both passes classify alike
  uint8_t* dst = a.out + (outpos - shift);
  const uint32_t end = shift + K;
  for (uint32_t lo = tid * 16; lo < end; lo += kThreads * 16) {
    if (lo >= shift && lo + 16 <= end) {
      *reinterpret_cast<uint4*>(dst + lo) = *reinterpret_cast<const uint4*>(stage + lo);
    } else {
      const uint32_t b0 = lo > shift ? lo : shift, b1 = lo + 16 < end ? lo + 16 : end;
      for (uint32_t b = b0; b < b1; b++) dst[b] = stage[b];
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_parse_compact_fasta(CompactArgs a) {
  __shared__ uint8_t sh_first[kThreads], sh_last[kThreads];
  __shared__ uint64_t sh64[8];
  __shared__ uint32_t sh32[4];
  __shared__ __attribute__((aligned(16))) uint8_t stage[kTile + 32];
  const uint32_t tid = threadIdx.x;
  const uint64_t tile = blockIdx.x;
  const ParseTileIn st = a.states[tile];
  const Chunk c = load_chunk(a.text - a.lead, a.lead, a.len, tile, tid);
  const Lines L = classify(c, a.len, a.text, sh_first, sh_last, tid);
  const uint32_t hdr = header_starts(c, L.ls);
  const bool has = L.ls != 0;
  const bool last_hdr = has && ((hdr >> (31 - __builtin_clz(L.ls))) & 1);
  uint32_t tile_last;
  const uint32_t enter = block_enter_class(has, last_hdr, st.cls, &tile_last, sh64, tid);
  const uint32_t in_hdr = header_bytes(L.ls, hdr, enter == kClsHdr);
  const uint32_t kept = L.content & ~in_hdr;
  uint32_t tot;
  const uint32_t ex = block_scan_excl(__builtin_popcount(kept) | (__builtin_popcount(hdr) << 16), &tot, sh32, tid);
  const uint32_t kbase = ex & 0xffffu;
  const uint64_t rbase = st.count + (ex >> 16);          // records that start in front of this chunk

  for (uint32_t m = hdr; m; m &= m - 1) {                // record starts
    const uint32_t j = __builtin_ctz(m);
    const uint64_t r = rbase + __builtin_popcount(hdr & below(j));
    if (r < a.n) {
      a.offsets[r] = st.outpos + kbase + __builtin_popcount(kept & below(j));
      a.name_start[r] = (uint64_t)(c.pos0 + j) + 1;
    }
  }
  for (uint32_t m = L.ends & in_hdr; m; m &= m - 1) {    // ends of header lines: where the name stops
    const uint32_t j = __builtin_ctz(m);
    const uint64_t r = rbase + __builtin_popcount(hdr & (below(j) | (1u << j))) - 1;
    const bool is_nl = (L.nl >> j) & 1;
    uint64_t end = (uint64_t)(c.pos0 + j);
    if (is_nl) end -= (L.cr_before >> j) & 1;
    else end += byte_of(c, j) == '\r' ? 0 : 1;           // the text's last byte: a '\r' there is the terminator
    if (r < a.n) a.name_end[r] = end;
  }
  if (rbase == 0) {                                      // sequence data in front of the first header
    const uint32_t bad = kept & (hdr ? below(__builtin_ctz(hdr)) : 0xffffu);
    if (bad) atomicMin(a.err, (unsigned long long)(c.pos0 + __builtin_ctz(bad)));
  }
  stage_and_store(c, kept, kbase, tot & 0xffffu, st.outpos, a, stage, tid);
}

__global__ __launch_bounds__(kThreads) void k_parse_compact_fastq(CompactArgs a) {
  __shared__ uint8_t sh_first[kThreads], sh_last[kThreads];
  __shared__ uint32_t sh32[4];
  __shared__ __attribute__((aligned(16))) uint8_t stage[kTile + 32];
  const uint32_t tid = threadIdx.x;
  const uint64_t tile = blockIdx.x;
  const ParseTileIn st = a.states[tile];
  const Chunk c = load_chunk(a.text - a.lead, a.lead, a.len, tile, tid);
  const Lines L = classify(c, a.len, a.text, sh_first, sh_last, tid);
  uint32_t t_nl, tot;
  const uint64_t line0 = st.count + block_scan_excl(__builtin_popcount(L.nl), &t_nl, sh32, tid);   // line of byte 0
  uint32_t seqm, qualm;
  fastq_roles(L.nl, L.content, (uint32_t)(line0 & 3), &seqm, &qualm);
  const uint32_t ex = block_scan_excl(__builtin_popcount(seqm) | (__builtin_popcount(qualm) << 16), &tot, sh32, tid);
  const uint32_t kbase = ex & 0xffffu;
  const int64_t bal0 = st.bal + (int64_t)kbase - (int64_t)(ex >> 16);

  for (uint32_t m = L.ls; m; m &= m - 1) {               // line starts: records, and the markers
    const uint32_t j = __builtin_ctz(m);
    const uint64_t line = line0 + __builtin_popcount(L.nl & below(j));
    if (line >= a.lines) break;                          // an empty line at the end of the text
    const uint32_t role = (uint32_t)(line & 3);
    const uint64_t r = line >> 2;
    if (role == 0) {
      if (r < a.n) {
        a.offsets[r] = st.outpos + kbase + __builtin_popcount(seqm & below(j));
        a.name_start[r] = (uint64_t)(c.pos0 + j) + 1;
      }
      if (byte_of(c, j) != '@') atomicMin(a.err, (unsigned long long)r);
    } else if (role == 2) {
      if (byte_of(c, j) != '+') atomicMin(a.err, (unsigned long long)r);
    }
  }
  for (uint32_t m = L.ends; m; m &= m - 1) {             // line ends: the name's end; sequence against quality
    const uint32_t j = __builtin_ctz(m);
    const uint64_t line = line0 + __builtin_popcount(L.nl & below(j));
    const uint32_t role = (uint32_t)(line & 3);
    const uint64_t r = line >> 2;
    if (role == 0) {
      const bool is_nl = (L.nl >> j) & 1;
      uint64_t end = (uint64_t)(c.pos0 + j);
      if (is_nl) end -= (L.cr_before >> j) & 1;
      else end += byte_of(c, j) == '\r' ? 0 : 1;
      if (r < a.n) a.name_end[r] = end;
    } else if (role == 3) {
      // the running balance (sequence bytes - quality bytes) is zero behind every sound record, so the lowest record
      // behind which it is not zero is the lowest one whose two lengths differ
      const uint32_t thru = below(j) | (1u << j);
      const int64_t bal = bal0 + __builtin_popcount(seqm & thru) - __builtin_popcount(qualm & thru);
      if (bal != 0) atomicMin(a.err, (unsigned long long)r);
    }
  }
  stage_and_store(c, seqm, kbase, tot & 0xffffu, st.outpos, a, stage, tid);
}

// the first content byte of the text (what SMH_FORMAT_AUTO looks at): *out = its value, or ~0 when there is none
__global__ __launch_bounds__(kThreads) void k_first_content(const uint8_t* text, uint64_t len, uint64_t* out) {
  __shared__ uint32_t found;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) { found = ~0u; *out = ~0ull; }
  __syncthreads();
  for (uint64_t base = 0; base < len; base += kThreads) {
    const uint64_t p = base + tid;
    if (p < len) {
      const uint8_t b = text[p];
      const bool term = b == '\n' || (b == '\r' && (p + 1 == len || text[p + 1] == '\n'));
      if (!term) atomicMin(&found, tid);
    }
    __syncthreads();
    const uint32_t f = found;
    __syncthreads();
    if (f != ~0u) {
      if (tid == 0) *out = text[base + f];
      return;
    }
  }
}

struct Layout { uint64_t ntiles, nblocks; size_t sums, states, agg, bytes; };
Layout layout_of(const void* text, uint64_t len) {
  Layout l;
  const uint64_t lead = (uintptr_t)text & 15;
  l.ntiles = (lead + len + kTile - 1) / kTile;
  l.nblocks = (l.ntiles + kThreads - 1) / kThreads;
  l.sums = 0;
  l.states = l.sums + ((l.ntiles * sizeof(TileSum) + 255) & ~(size_t)255);
  l.agg = l.states + ((l.ntiles * sizeof(ParseTileIn) + 255) & ~(size_t)255);
  l.bytes = l.agg + l.nblocks * sizeof(FastqScan::Elem) + 256;
  return l;
}

template <class S>
void run_scan(const Layout& l, uint8_t* ws, const ParseTileIn& first, ParseTotals* totals_dev, hipStream_t s) {
  auto* sums = reinterpret_cast<const TileSum*>(ws + l.sums);
  auto* states = reinterpret_cast<ParseTileIn*>(ws + l.states);
  auto* agg = reinterpret_cast<typename S::Elem*>(ws + l.agg);
  k_scan_reduce<S><<<dim3((uint32_t)l.nblocks), dim3(kThreads), 0, s>>>(sums, l.ntiles, agg);
  k_scan_top<S><<<dim3(1), dim3(kThreads), 0, s>>>(agg, l.nblocks, first, totals_dev);
  k_scan_down<S><<<dim3((uint32_t)l.nblocks), dim3(kThreads), 0, s>>>(sums, l.ntiles, agg, first, states);
}

}  // namespace

size_t parse_workspace_bytes(const void* text, uint64_t len) { return layout_of(text, len).bytes; }

void launch_first_content(const uint8_t* text, uint64_t len, uint64_t* out_dev, hipStream_t s) {
  k_first_content<<<dim3(1), dim3(kThreads), 0, s>>>(text, len, out_dev);
  HIP_CHECK(hipGetLastError());
}

void launch_parse_scan(int format, const uint8_t* text, uint64_t len, const ParseTileIn& first, void* workspace,
                       ParseTotals* totals_dev, hipStream_t s) {
  const Layout l = layout_of(text, len);
  if (l.ntiles == 0 || l.ntiles > 0xffffffffull) throw_internal("parse: text length out of range");
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  auto* sums = reinterpret_cast<TileSum*>(ws + l.sums);
  const uint32_t lead = (uint32_t)((uintptr_t)text & 15);
  if (format == kFormatFasta) {
    k_parse_summary_fasta<<<dim3((uint32_t)l.ntiles), dim3(kThreads), 0, s>>>(text, lead, len, sums);
    run_scan<FastaScan>(l, ws, first, totals_dev, s);
  } else {
    k_parse_summary_fastq<<<dim3((uint32_t)l.ntiles), dim3(kThreads), 0, s>>>(text, lead, len, sums);
    run_scan<FastqScan>(l, ws, first, totals_dev, s);
  }
  HIP_CHECK(hipGetLastError());
}

void launch_parse_compact(int format, const uint8_t* text, uint64_t len, const void* workspace, const ParseTotals& totals,
                          uint8_t* out, uint64_t* offsets_dev, uint64_t* name_start_dev, uint64_t* name_end_dev,
                          ParseTotals* totals_dev, hipStream_t s) {
  const Layout l = layout_of(text, len);
  if ((uintptr_t)out & 15) throw_internal("parse: output buffer is not 16-byte aligned");
  CompactArgs a;
  a.text = text; a.lead = (uint32_t)((uintptr_t)text & 15); a.len = len;
  a.states = reinterpret_cast<const ParseTileIn*>(static_cast<const uint8_t*>(workspace) + l.states);
  a.out = out; a.offsets = offsets_dev; a.name_start = name_start_dev; a.name_end = name_end_dev;
  a.n = totals.n_records; a.total = totals.total; a.lines = totals.lines;
  a.err = reinterpret_cast<unsigned long long*>(&totals_dev->err);
  if (format == kFormatFasta) k_parse_compact_fasta<<<dim3((uint32_t)l.ntiles), dim3(kThreads), 0, s>>>(a);
  else k_parse_compact_fastq<<<dim3((uint32_t)l.ntiles), dim3(kThreads), 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace smh
