// sketch_kernels.hip -- what the arms of KmerMinHash::add_sequence (reference src/lib.rs:252-305) share on the launch
// side, and the sketch kernels that belong to no arm.  The arms are sketch_dna_kernels.hip, sketch_protein_kernels.hip and
// sketch_amino_kernels.hip; their shared device code is murmur_device.hpp and sketch_device.hpp, their shared host code
// sketch_launch.hpp.
//
//   k_tile_records     record (and the end of its valid part) of every launch tile's first position, so that no lane
//                      searches all record starts (with_tile_records, called by the launchers of the tiled kernels).
//   k_hash_segments    murmur64 of whole byte strings (add_word lib.rs:247-250, ffi.rs:15-24).
//   k_filter_hashes    add_many in bulk (lib.rs:412-417): the filter and the append on hashes that exist.
//   k_synth_dna        benchmark input generator.
//
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

// the per-tile record table of the tiled kernels (sketch_device.hpp: find_record_in_tile)
__global__ __launch_bounds__(256) void k_tile_records(const uint64_t* __restrict__ starts, const uint64_t* __restrict__ vends,
                                                      uint32_t nrec, uint32_t min_len, uint64_t base, uint64_t tile,
                                                      uint64_t ntiles, TileRec* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntiles) return;
  const uint32_t r = find_record(starts, nrec, base + t * tile);
  out[t] = TileRec{r, find_record(starts, nrec, base + (t + 1) * tile), record_valid_end(starts, vends, min_len, r)};
}

__global__ __launch_bounds__(256) void k_hash_segments(const uint8_t* __restrict__ bytes,
                                                       const uint64_t* __restrict__ off, uint32_t nseg,
                                                       uint64_t seed, uint64_t* __restrict__ out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nseg) return;
  Mm3Stream st(seed);
  for (uint64_t q = off[i]; q < off[i + 1]; q++) st.push(bytes[q]);
  out[i] = st.finish();
}

// ---------------------------------------------------------------------------------
// add_many (reference src/lib.rs:412-417) in bulk: the hashes already exist, only the filter and
// the append remain; the stream position of hash i is i.
__global__ __launch_bounds__(256) void k_filter_hashes(const uint64_t* __restrict__ hashes, HashParams hp, CandSink sink) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t thr = hp.thr;
  for (uint64_t i = hp.range_lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hp.range_hi; i += stride) {
    const uint64_t h = hashes[i];
    if (h <= thr) emit(sink, h, hp.pos_base + i);
  }
}

// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t seed, uint64_t index) {
  uint64_t z = seed + (index + 1) * 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// one lane per 64-bit generator word = 32 bases; `start` is a multiple of 32
__global__ __launch_bounds__(256) void k_synth_dna(uint8_t* __restrict__ out, uint64_t start, uint64_t len,
                                                   uint64_t seed, uint64_t n_every) {
  const uint64_t nwords = (len + 31) / 32;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += stride) {
    uint64_t bits = splitmix64(seed, (start >> 5) + w);
    uint64_t p = start + 32 * w;
    uint64_t nrem = n_every ? p % n_every : 0;
    uint64_t o = 32 * w;
    for (int j = 0; j < 32 && o + j < len; j++) {
      uint32_t c = (0x54474341u >> (8 * ((bits >> (2 * j)) & 3))) & 0xffu;
      if (n_every) {
        if (nrem == n_every - 1) c = 'N';
        nrem = nrem + 1 == n_every ? 0 : nrem + 1;
      }
      out[o + j] = (uint8_t)c;
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------------
// launchers

// the batch with its per-tile record table (k_tile_records) for a launch of `ntiles` tiles from position `base`
SeqBatch with_tile_records(const SeqBatch& b, uint32_t min_len, uint64_t base, uint64_t tile, uint64_t ntiles, Device& dev,
                           hipStream_t s) {
  SeqBatch r = b;
  if (!b.starts || b.nrec < 2) return r;
  dev.tile_rec.ensure((size_t)ntiles * sizeof(TileRec));
  hipLaunchKernelGGL(k_tile_records, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, s, b.starts, b.vends, b.nrec, min_len, base,
                     tile, ntiles, dev.tile_rec.as<TileRec>());
  r.tile_rec = dev.tile_rec.as<TileRec>();
  return r;
}

void launch_hash_segments(const uint8_t* bytes, const uint64_t* seg_offsets, uint32_t nseg,
                          uint64_t seed, uint64_t* out, hipStream_t s) {
  if (nseg == 0) return;
  hipLaunchKernelGGL(k_hash_segments, dim3((nseg + 255) / 256), dim3(256), 0, s, bytes, seg_offsets,
                     nseg, seed, out);
  HIP_CHECK(hipGetLastError());
}

void launch_filter_hashes(const uint64_t* hashes, const HashParams& p, const CandSink& sink, hipStream_t s) {
  if (p.range_hi <= p.range_lo) return;
  hipLaunchKernelGGL(k_filter_hashes, dim3(sketch_grid(p.range_hi - p.range_lo, 256, 4096)), dim3(256), 0, s, hashes, p, sink);
  HIP_CHECK(hipGetLastError());
}

void launch_synth_dna(uint8_t* out, uint64_t start, uint64_t len, uint64_t seed, uint64_t n_every,
                      hipStream_t s) {
  if (len == 0) return;
  if (start & 31) throw_internal("synth_dna: start must be a multiple of 32");
  hipLaunchKernelGGL(k_synth_dna, dim3(sketch_grid((len + 31) / 32, 256, 8192)), dim3(256), 0, s, out,
                     start, len, seed, n_every);
  HIP_CHECK(hipGetLastError());
}

}  // namespace smh
