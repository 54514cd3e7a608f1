// sketch_device.hpp -- device code shared by the sketch kernels' translation units (sketch_kernels.hip,
// sketch_dna_kernels.hip, sketch_protein_kernels.hip, sketch_amino_kernels.hip): the candidate sink's emit, the LDS stage
// of a workgroup's survivors, the record look-ups (the per-tile table is written by k_tile_records, sketch_kernels.hip)
// and the upper-casing of a byte.  No state: everything is __device__ __forceinline__.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace smh {

__device__ __forceinline__ void emit(const CandSink& sink, uint64_t h, uint64_t pos) {
  unsigned long long idx = atomicAdd(sink.count, 1ull);  // hipcc aggregates this per wave
  if (idx < sink.capacity) {
    sink.hash[idx] = h;
    if (sink.pos) sink.pos[idx] = pos;
  }
}

// Survivors are staged in LDS and every workgroup flushes with ONE global atomic + coalesced
// stores: a per-wave global atomic on the single counter word saturates at ~88 M atomics/s
// (MI355X_MICROARCH.md "dequeue") and capped the DNA kernel at 84 G k-mers/s.
struct Stage {
  uint32_t* ctl;   // [0] = count, [2..3] = flush base
  uint64_t* hash;
  uint64_t* pos;   // valid when the sink wants positions
  uint32_t cap;
};
__device__ __forceinline__ void stage_emit(const Stage& st, const CandSink& sink, uint64_t h, uint64_t pos) {
  const uint32_t slot = atomicAdd(&st.ctl[0], 1u);  // LDS atomic
  if (slot < st.cap) { st.hash[slot] = h; if (sink.pos) st.pos[slot] = pos; }
  else emit(sink, h, pos);                          // stage full: straight to the global sink
}
// all threads of the workgroup must call this (it synchronises).  Nothing is written while fewer
// than `at_least` survivors are staged (0 = flush whatever is there).
__device__ __forceinline__ void stage_flush(const Stage& st, const CandSink& sink, int tid, int nthreads,
                                            uint32_t at_least = 0) {
  __syncthreads();
  const uint32_t staged = min(st.ctl[0], st.cap);
  if (staged && staged >= at_least) {
    if (tid == 0) {
      unsigned long long base = atomicAdd(sink.count, (unsigned long long)staged);
      st.ctl[2] = (uint32_t)base; st.ctl[3] = (uint32_t)(base >> 32);
    }
    __syncthreads();
    const uint64_t base = ((uint64_t)st.ctl[3] << 32) | st.ctl[2];
    for (uint32_t e = tid; e < staged; e += nthreads)
      if (base + e < sink.capacity) {
        sink.hash[base + e] = st.hash[e];
        if (sink.pos) sink.pos[base + e] = st.pos[e];
      }
    __syncthreads();
    if (tid == 0) st.ctl[0] = 0;
  }
}

// last record whose start is <= p   (starts has nrec+1 entries, starts[nrec] = total length)
__device__ __forceinline__ uint32_t find_record(const uint64_t* __restrict__ starts, uint32_t nrec,
                                                uint64_t p) {
  uint32_t lo = 0, hi = nrec;  // answer in [lo, hi)
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (starts[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// The tiled kernels need, per lane, the record its run starts in and where that record's valid part ends.  A binary
// search over all record starts is ~log2(nrec) DEPENDENT global loads that every lane of a workgroup waits for at the
// top of every tile (14 at 10 000 records: a tenth of the tile's time), and their misses show up as memory requests.
// One tiny launch looks up the record of every TILE's first position instead, with its end; a lane reads its tile's
// entry (one 16-byte load, the same for the whole workgroup) and is done when the tile lies inside one record; otherwise
// it searches between the entry's two record numbers.
// end of the valid part of record r: vends[r] when given (DNA arm, force=false); a record shorter than min_len adds
// nothing (protein arm, src/lib.rs:257)
__device__ __forceinline__ uint64_t record_valid_end(const uint64_t* __restrict__ starts, const uint64_t* __restrict__ vends,
                                                     uint32_t min_len, uint32_t r) {
  if (vends) return vends[r];
  const uint64_t s0 = starts[r], s1 = starts[r + 1];
  return (min_len && s1 - s0 < min_len) ? s0 : s1;
}
// record of position p, known to lie in tile `tix` of the launch, and the end of its valid part
// (min_len by reference, so that what a kernel is compiled to does not depend on who else calls this in its translation
// unit: a value every caller of the unit passes as the same constant -- the DNA arm's 0 -- would be folded in here before
// the inlining, and k_dna_rolling then comes out with other registers and spills than next to the protein arm's caller;
// through the reference it is folded in the kernel, after the inlining, as ever.  profiles/r27_sketch_split_resources.txt)
__device__ __forceinline__ uint32_t find_record_in_tile(const SeqBatch& b, const uint32_t& min_len, uint64_t tix, uint64_t p,
                                                        uint64_t* end) {
  uint32_t lo = 0, hi = b.nrec;                            // answer in [lo, hi)
  if (b.tile_rec) {
    const TileRec t = b.tile_rec[tix];
    if (t.last == t.rec) { *end = t.end; return t.rec; }
    lo = t.rec; hi = t.last + 1;
  }
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (b.starts[mid] <= p) lo = mid; else hi = mid;
  }
  *end = record_valid_end(b.starts, b.vends, min_len, lo);
  return lo;
}

__device__ __forceinline__ uint32_t upper(uint32_t c) { return (c >= 'a' && c <= 'z') ? c - 32 : c; }

}  // namespace smh
