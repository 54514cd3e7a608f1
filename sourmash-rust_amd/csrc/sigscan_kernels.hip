// sigscan_kernels.hip -- signature JSON text resident in HBM -> the u64 values of its number arrays, the span table and the
// skeleton (the text without the spans' bytes), and the checks of an index gathered from the values.  DESIGN.md 3.27; the
// rules every byte follows are sigscan_core.hpp's automaton of eight states.
//
//   1. k_sig_summary   per tile of kSigTileBytes: the tile as a function of the state it is entered in -- the map of the eight
//                      states it leaves behind, and per entering state the skeleton bytes kept, spans opened and tokens started;
//   2. k_sig_scan_*    the ordered scan.  Maps compose (not commutative): reduce, top, down give every tile the state it is
//                      really entered in, which selects its three counts; a second reduce / top of plain 64-bit sums gives
//                      every tile its places in the skeleton, the span table and the values;
//   3. k_sig_compact   the same classification again with the entering state known: kept bytes to the skeleton, a '[' writes
//                      its span's start and first token, the byte that ends a span writes its end, a token's first digit
//                      parses the token (up to 21 digits, wherever they lie) and stores the value, rule breaks lower the span's
//                      offsets with atomicMin.
// Tiles are cut on 16-byte boundaries of the ADDRESS, so every full chunk is one aligned 16-byte load whatever the alignment
// of the text pointer; the chunks that hold the text's first and last bytes are read byte by byte and nothing outside
// [text, text + len) is touched.  Every kernel walks its tiles in a gridDim-stride loop (grid_for).
#include "kernels.hpp"
#include "sigscan_core.hpp"

namespace smh {

namespace {

using namespace sigscan;

constexpr uint32_t kThreads = kSigThreads;
constexpr uint32_t kTile = kSigTileBytes;
static_assert(kTile == kThreads * 16, "one 16-byte chunk per thread");

// one thread's 16 bytes: b[lo, hi) are bytes of the text
struct Chunk {
  uint8_t b[16];
  uint32_t lo, hi;
  uint64_t off;   // the text offset of b[0] (may lie in front of the text: then lo > 0)
};

__device__ __forceinline__ Chunk load_chunk(const uint8_t* text, uint32_t lead, uint64_t len, uint64_t tile, uint32_t tid) {
  Chunk c;
  const uint64_t v = tile * kTile + (uint64_t)tid * 16;   // position in the aligned address range that begins at text - lead
  c.off = v - lead;                                        // (wraps below zero for the first chunk: only b[lo..] is used)
  const uint64_t end = (uint64_t)lead + len;
  c.lo = v < lead ? (uint32_t)(lead - v < 16 ? lead - v : 16) : 0;
  c.hi = v >= end ? 0 : (end - v < 16 ? (uint32_t)(end - v) : 16);
  if (c.lo > c.hi) c.lo = c.hi;
  if (c.lo == 0 && c.hi == 16) {
    const uint4 w = *reinterpret_cast<const uint4*>(text - lead + v);
    const uint32_t q[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) c.b[i] = (uint8_t)(q[i >> 2] >> (8 * (i & 3)));
  } else {
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) c.b[i] = (i >= c.lo && i < c.hi) ? text[c.off + i] : 0;
  }
  return c;
}

// The chunk as a function of the state it is entered in: bits 0-2 the state left behind, 3-7 bytes kept, 8-12 spans opened,
// 13-17 tokens started.
__device__ __forceinline__ void chunk_table(const Chunk& c, uint32_t* pk) {
#pragma unroll
  for (uint32_t e = 0; e < kStates; e++) {
    uint32_t st = e, kept = 0, opens = 0, toks = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
      if (i >= c.lo && i < c.hi) {
        const Step s = step(st, c.b[i]);
        st = s.next;
        kept += (s.events & kKept) ? 1 : 0;
        opens += (s.events & kOpens) ? 1 : 0;
        toks += (s.events & kTokStart) ? 1 : 0;
      }
    }
    pk[e] = st | kept << 3 | opens << 8 | toks << 13;
  }
}

// a map of the eight states: three bits per entering state
constexpr uint32_t kIdentityMap = 0 | 1 << 3 | 2 << 6 | 3 << 9 | 4 << 12 | 5 << 15 | 6 << 18 | 7 << 21;
__device__ __forceinline__ uint32_t map_of(const uint32_t* pk) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t e = 0; e < kStates; e++) m |= (pk[e] & 7) << (3 * e);
  return m;
}
__device__ __forceinline__ uint32_t map_at(uint32_t m, uint32_t e) { return (m >> (3 * e)) & 7; }
// first `a`, then `b`
__device__ __forceinline__ uint32_t compose(uint32_t a, uint32_t b) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t e = 0; e < kStates; e++) m |= map_at(b, map_at(a, e)) << (3 * e);
  return m;
}

// inclusive scan of one map per thread over the workgroup, order kept; returns this thread's inclusive map.  sh: kThreads words.
__device__ __forceinline__ uint32_t block_scan_maps(uint32_t v, uint32_t* sh, uint32_t tid) {
  sh[tid] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kThreads; d <<= 1) {
    uint32_t o = v;
    if (tid >= d) o = compose(sh[tid - d], v);
    __syncthreads();
    v = o;
    sh[tid] = v;
    __syncthreads();
  }
  return v;
}

// inclusive prefix sum of one 64-bit word per thread.  sh: kThreads qwords.
__device__ __forceinline__ uint64_t block_scan_sum(uint64_t v, uint64_t* sh, uint32_t tid) {
  sh[tid] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kThreads; d <<= 1) {
    uint64_t o = v;
    if (tid >= d) o = sh[tid - d] + v;
    __syncthreads();
    v = o;
    sh[tid] = v;
    __syncthreads();
  }
  return v;
}

// per tile: the map, and per entering state kept | opens << 16 | toks << 32 (each at most 4096)
struct TileSum { uint64_t cnt[kStates]; uint32_t map, pad; };
struct Counts { uint64_t kept, opens, toks; };

// ---------------------------------------------------------------------------------------------------------------
// pass 1

__global__ __launch_bounds__(kThreads) void k_sig_summary(const uint8_t* text, uint32_t lead, uint64_t len, uint64_t ntiles, TileSum* sums) {
  __shared__ uint32_t sh[kThreads];
  __shared__ unsigned long long acc[kStates];
  const uint32_t tid = threadIdx.x;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const Chunk c = load_chunk(text, lead, len, tile, tid);
    uint32_t pk[kStates];
    chunk_table(c, pk);
    if (tid < kStates) acc[tid] = 0;
    const uint32_t incl = block_scan_maps(map_of(pk), sh, tid);   // (its barriers also publish acc)
    const uint32_t excl = tid ? sh[tid - 1] : kIdentityMap;
    // the thread's counts for every state the TILE may be entered in, summed over the workgroup: wave first, then LDS
#pragma unroll
    for (uint32_t e = 0; e < kStates; e++) {
      const uint32_t q = pk[map_at(excl, e)];
      uint64_t w = (uint64_t)((q >> 3) & 31) | (uint64_t)((q >> 8) & 31) << 16 | (uint64_t)((q >> 13) & 31) << 32;
      for (uint32_t d = 32; d; d >>= 1) w += __shfl_xor(w, d, 64);
      if ((tid & 63) == 0) atomicAdd(&acc[e], (unsigned long long)w);
    }
    __syncthreads();
    if (tid < kStates) sums[tile].cnt[tid] = acc[tid];
    if (tid == kThreads - 1) { sums[tile].map = incl; sums[tile].pad = 0; }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------
// pass 2.  Blocks of kThreads tiles; nblocks = ceil(ntiles / kThreads).

__global__ __launch_bounds__(kThreads) void k_sig_scan_reduce(const TileSum* sums, uint64_t ntiles, uint64_t nblocks, uint32_t* agg_map) {
  __shared__ uint32_t sh[kThreads];
  const uint32_t tid = threadIdx.x;
  for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const uint64_t i = b * kThreads + tid;
    const uint32_t incl = block_scan_maps(i < ntiles ? sums[i].map : kIdentityMap, sh, tid);
    if (tid == kThreads - 1) agg_map[b] = incl;
    __syncthreads();
  }
}

// one workgroup: agg_map[b] -> the state block b is entered in (the text is entered in kOut)
__global__ __launch_bounds__(kThreads) void k_sig_scan_top(uint32_t* agg_map, uint64_t nblocks) {
  __shared__ uint32_t sh[kThreads];
  const uint32_t tid = threadIdx.x;
  uint32_t carry = kIdentityMap;
  for (uint64_t base = 0; base < nblocks; base += kThreads) {
    const uint64_t i = base + tid;
    block_scan_maps(i < nblocks ? agg_map[i] : kIdentityMap, sh, tid);
    const uint32_t excl = tid ? compose(carry, sh[tid - 1]) : carry;
    const uint32_t next = compose(carry, sh[kThreads - 1]);
    __syncthreads();
    if (i < nblocks) agg_map[i] = map_at(excl, kOut);
    carry = next;
  }
}

// the state every tile is entered in, its counts' prefix inside the block, and the block's sums
__global__ __launch_bounds__(kThreads) void k_sig_scan_down(const TileSum* sums, uint64_t ntiles, uint64_t nblocks, const uint32_t* block_state,
                                                            uint32_t* tile_state, Counts* tile_base, Counts* agg_cnt) {
  __shared__ uint32_t sh[kThreads];
  __shared__ uint64_t sh64[kThreads];
  const uint32_t tid = threadIdx.x;
  for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const uint64_t i = b * kThreads + tid;
    block_scan_maps(i < ntiles ? sums[i].map : kIdentityMap, sh, tid);
    const uint32_t st = map_at(tid ? sh[tid - 1] : kIdentityMap, block_state[b]);
    const uint64_t w = i < ntiles ? sums[i].cnt[st] : 0;
    Counts in;
    const uint64_t part[3] = {w & 0xffff, (w >> 16) & 0xffff, (w >> 32) & 0xffff};
    uint64_t incl[3];
    for (uint32_t k = 0; k < 3; k++) {
      __syncthreads();
      incl[k] = block_scan_sum(part[k], sh64, tid);
    }
    in.kept = incl[0] - part[0]; in.opens = incl[1] - part[1]; in.toks = incl[2] - part[2];
    if (i < ntiles) { tile_state[i] = st; tile_base[i] = in; }
    if (tid == kThreads - 1) agg_cnt[b] = Counts{incl[0], incl[1], incl[2]};
    __syncthreads();
  }
}

// one workgroup: agg_cnt[b] -> the counts in front of block b; the totals and the state the text ends in
__global__ __launch_bounds__(kThreads) void k_sig_scan_top2(Counts* agg_cnt, uint64_t nblocks, const TileSum* sums, const uint32_t* tile_state,
                                                            uint64_t ntiles, SigTotals* totals) {
  __shared__ uint64_t sh64[kThreads];
  const uint32_t tid = threadIdx.x;
  uint64_t carry[3] = {0, 0, 0};
  for (uint64_t base = 0; base < nblocks; base += kThreads) {
    const uint64_t i = base + tid;
    const Counts c = i < nblocks ? agg_cnt[i] : Counts{0, 0, 0};
    const uint64_t part[3] = {c.kept, c.opens, c.toks};
    uint64_t excl[3];
    for (uint32_t k = 0; k < 3; k++) {
      __syncthreads();
      const uint64_t incl = block_scan_sum(part[k], sh64, tid);
      excl[k] = carry[k] + incl - part[k];
      carry[k] += sh64[kThreads - 1];
    }
    __syncthreads();
    if (i < nblocks) agg_cnt[i] = Counts{excl[0], excl[1], excl[2]};
  }
  if (tid == 0) {
    totals->skeleton = carry[0]; totals->spans = carry[1]; totals->tokens = carry[2];
    totals->final_state = ntiles ? map_at(sums[ntiles - 1].map, tile_state[ntiles - 1]) : (uint32_t)kOut;
    totals->pad = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// pass 3

struct CompactArgs {
  const uint8_t* text; uint32_t lead; uint64_t len, ntiles;
  const uint32_t* tile_state; const Counts* tile_base; const Counts* block_base;
  uint8_t* skeleton; SigSpanDev* rows; uint64_t* values;
  uint64_t n_skeleton, n_spans, n_tokens;
};

__global__ __launch_bounds__(kThreads) void k_sig_compact(CompactArgs a) {
  __shared__ uint32_t sh[kThreads];
  __shared__ uint64_t sh64[kThreads];
  const uint32_t tid = threadIdx.x;
  for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const Chunk c = load_chunk(a.text, a.lead, a.len, tile, tid);
    uint32_t pk[kStates];
    chunk_table(c, pk);
    block_scan_maps(map_of(pk), sh, tid);
    uint32_t st = map_at(tid ? sh[tid - 1] : kIdentityMap, a.tile_state[tile]);
    const uint32_t q = pk[st];
    const uint64_t mine = (uint64_t)((q >> 3) & 31) | (uint64_t)((q >> 8) & 31) << 16 | (uint64_t)((q >> 13) & 31) << 32;
    __syncthreads();
    const uint64_t front = block_scan_sum(mine, sh64, tid) - mine;
    const Counts tb = a.tile_base[tile], bb = a.block_base[tile / kThreads];
    uint64_t kept = tb.kept + bb.kept + (front & 0xffff);
    uint64_t span = tb.opens + bb.opens + ((front >> 16) & 0xffff);   // spans opened in front of the next byte
    uint64_t tok = tb.toks + bb.toks + ((front >> 32) & 0xffff);
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
      if (i < c.lo || i >= c.hi) continue;
      const uint64_t at = c.off + i;
      const uint32_t before = st;
      const Step s = step(st, c.b[i]);
      st = s.next;
      // (every index is checked against the counts the scan gave: a disagreement of the two passes must not write outside)
      if ((s.events & kSpanEnd) && span - 1 < a.n_spans) {
        SigSpanDev& r = a.rows[span - 1];
        r.end = at; r.end_token = tok; r.last_state = before;
      }
      if ((s.events & kKept) && kept < a.n_skeleton) a.skeleton[kept] = c.b[i];
      kept += (s.events & kKept) ? 1 : 0;
      if (s.events & kOpens) {
        if (span < a.n_spans) { SigSpanDev& r = a.rows[span]; r.start = at + 1; r.first_token = tok; }
        span++;
      }
      if ((s.events & kBad) && span - 1 < a.n_spans) atomicMin(reinterpret_cast<unsigned long long*>(&a.rows[span - 1].bad_syntax), (unsigned long long)at);
      if (s.events & kTokStart) {
        const Token t = parse_token(a.text + at, a.len - at);
        if (tok < a.n_tokens) a.values[tok] = t.value;
        tok++;
        if (t.flaw != kFlawNone && span - 1 < a.n_spans) {
          SigSpanDev& r = a.rows[span - 1];
          atomicMin(reinterpret_cast<unsigned long long*>(t.flaw == kFlawLeadingZero ? &r.bad_syntax : &r.overflow), (unsigned long long)at);
        }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------
// the checks of a gathered index

__device__ __forceinline__ uint32_t node_of(const uint64_t* off, uint32_t n, uint64_t i) {   // off[s] <= i < off[s + 1]
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// hashes: the gathered CSR.  *err is lowered to node << 32 | position by every hash that is not above the one in front of it
// in its node.  With abundances: out_abunds[i] = the abundance narrowed to 32 bits; one of 2^32 or more is stored as all ones
// and counted in *n_wide, and -- when wide_pos is given -- its place i is appended there (any order, at most wide_cap).
__global__ __launch_bounds__(256) void k_sig_gather_check(const uint64_t* hashes, const uint64_t* off, uint32_t n, uint64_t total,
                                                          const uint64_t* values, const uint64_t* abund_src, uint32_t* out_abunds,
                                                          unsigned long long* err, unsigned long long* n_wide, uint64_t* wide_pos,
                                                          uint64_t wide_cap) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint32_t s = node_of(off, n, i);
    const uint64_t t = i - off[s];
    if (t && hashes[i - 1] >= hashes[i]) atomicMin(err, (unsigned long long)s << 32 | (t > 0xffffffffull ? 0xffffffffull : t));
    if (out_abunds) {
      uint64_t ab = values[abund_src[s] + t];
      if (ab >> 32) {
        const unsigned long long k = atomicAdd(n_wide, 1ull);
        if (wide_pos && k < wide_cap) wide_pos[k] = i;
        ab = 0xffffffffull;
      }
      out_abunds[i] = (uint32_t)ab;
    }
  }
}

struct Layout { uint64_t ntiles, nblocks; size_t sums, state, base, agg_map, agg_cnt, bytes; };
Layout layout_of(const void* text, uint64_t len) {
  Layout l;
  const uint64_t lead = (uintptr_t)text & 15;
  l.ntiles = (lead + len + kTile - 1) / kTile;
  l.nblocks = (l.ntiles + kThreads - 1) / kThreads;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  l.sums = 0;
  l.state = l.sums + up(l.ntiles * sizeof(TileSum));
  l.base = l.state + up(l.ntiles * 4);
  l.agg_map = l.base + up(l.ntiles * sizeof(Counts));
  l.agg_cnt = l.agg_map + up(l.nblocks * 4);
  l.bytes = l.agg_cnt + up(l.nblocks * sizeof(Counts)) + 256;
  return l;
}

}  // namespace

void sigscan_geometry(uint32_t* tile_bytes, uint32_t* threads) {
  if (tile_bytes) *tile_bytes = kTile;
  if (threads) *threads = kThreads;
}

size_t sigscan_workspace_bytes(const void* text, uint64_t len) { return layout_of(text, len).bytes; }

void launch_sigscan_scan(const uint8_t* text, uint64_t len, void* workspace, SigTotals* totals_dev, Device& dev, hipStream_t s) {
  const Layout l = layout_of(text, len);
  if (l.ntiles == 0 || l.ntiles > 0xffffffffull) throw_internal("sigscan: text length out of range");
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  auto* sums = reinterpret_cast<TileSum*>(ws + l.sums);
  auto* state = reinterpret_cast<uint32_t*>(ws + l.state);
  auto* base = reinterpret_cast<Counts*>(ws + l.base);
  auto* agg_map = reinterpret_cast<uint32_t*>(ws + l.agg_map);
  auto* agg_cnt = reinterpret_cast<Counts*>(ws + l.agg_cnt);
  const uint32_t lead = (uint32_t)((uintptr_t)text & 15);
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_sig_summary, dim3(grid_for(l.ntiles, 1, dev.grid_limit(), dev)), dim3(kThreads), 0, s, text, lead, len, l.ntiles, sums);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("sigscan_summary", s);
  dev.prof_begin(s);
  const dim3 grid(grid_for(l.nblocks, 1, dev.grid_limit(), dev));
  hipLaunchKernelGGL(k_sig_scan_reduce, grid, dim3(kThreads), 0, s, sums, l.ntiles, l.nblocks, agg_map);
  hipLaunchKernelGGL(k_sig_scan_top, dim3(1), dim3(kThreads), 0, s, agg_map, l.nblocks);
  hipLaunchKernelGGL(k_sig_scan_down, grid, dim3(kThreads), 0, s, sums, l.ntiles, l.nblocks, agg_map, state, base, agg_cnt);
  hipLaunchKernelGGL(k_sig_scan_top2, dim3(1), dim3(kThreads), 0, s, agg_cnt, l.nblocks, sums, state, l.ntiles, totals_dev);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("sigscan_scan", s);
}

void launch_sigscan_compact(const uint8_t* text, uint64_t len, const void* workspace, const SigTotals& totals, uint8_t* skeleton,
                            SigSpanDev* rows, uint64_t* values, Device& dev, hipStream_t s) {
  const Layout l = layout_of(text, len);
  const uint8_t* ws = static_cast<const uint8_t*>(workspace);
  CompactArgs a;
  a.text = text; a.lead = (uint32_t)((uintptr_t)text & 15); a.len = len; a.ntiles = l.ntiles;
  a.tile_state = reinterpret_cast<const uint32_t*>(ws + l.state);
  a.tile_base = reinterpret_cast<const Counts*>(ws + l.base);
  a.block_base = reinterpret_cast<const Counts*>(ws + l.agg_cnt);
  a.skeleton = skeleton; a.rows = rows; a.values = values;
  a.n_skeleton = totals.skeleton; a.n_spans = totals.spans; a.n_tokens = totals.tokens;
  dev.prof_begin(s);
  hipLaunchKernelGGL(k_sig_compact, dim3(grid_for(l.ntiles, 1, dev.grid_limit(), dev)), dim3(kThreads), 0, s, a);
  HIP_CHECK(hipGetLastError());
  dev.prof_end("sigscan_compact", s);
}

void launch_sigscan_gather_check(const uint64_t* hashes, const uint64_t* offsets_dev, uint32_t n, uint64_t total, const uint64_t* values,
                                 const uint64_t* abund_src_dev, uint32_t* out_abunds, unsigned long long* err, unsigned long long* n_wide,
                                 uint64_t* wide_pos, uint64_t wide_cap, Device& dev, hipStream_t s) {
  if (n == 0 || total == 0) return;
  hipLaunchKernelGGL(k_sig_gather_check, dim3(grid_for(total, 256, dev.grid_limit(), dev)), dim3(256), 0, s, hashes, offsets_dev, n, total, values,
                     abund_src_dev, out_abunds, err, n_wide, wide_pos, wide_cap);
  HIP_CHECK(hipGetLastError());
}

}  // namespace smh
