// archive_kernels.hip -- the members of a zip collection inflated on the device.  Three kernels, queued one
// behind the other on the call's stream:
//   k_inflate_queue    one wave per inflated member (the decoder of inflate_core.hpp, run lane-uniform into the sink of
//                      wave_sink.hpp, exactly as k_inflate runs it), but the members are NOT walked in a grid-stride order:
//                      a wave draws a ticket -- an atomicAdd on a zeroed word made by ALL lanes in uniform control flow, lane 0
//                      adding one and the others nothing, lane 0's old value broadcast; NOT `if (lane == 0) atomicAdd`, which
//                      hung on the device (see the loop) -- and takes order[ticket], the members sorted by payload length
//                      descending.  Members differ by orders
//                      of magnitude here and one wave decodes a few MB/s: the longest member is started first, and no wave
//                      is bound to members it has not started.  No CRC: a multi-megabyte text is not checked by one wave.
//   k_archive_chunks   one wave per chunk of archive::kChunk bytes of text; the wave finds its member by bisecting the chunk
//                      prefix.  A stored member's chunk is first copied from the entry's bytes.  The chunk's CRC register
//                      from state 0 goes to terms[chunk].
//   k_archive_crc      one wave per member folds the member's chunk registers (archive::fold_lane_term), compares with the
//                      expected CRC-32 and, on a mismatch, sets kCrc and lowers the call's error word as k_inflate does.
// A kernel boundary stands between the decoder's stores and the reads of the chunk kernel, and between the chunk registers
// and the fold.  Every offset into the text is 64-bit: the pointers are advanced by out_off before a 32-bit position is added.
#include "archive_core.hpp"
#include "kernels.hpp"
#include "wave_sink.hpp"

namespace smh {

namespace {

constexpr uint32_t kWavesPerBlock = kInflateThreads / 64;

__device__ inline uint32_t wave_xor(uint32_t x) {
  for (int d = 32; d; d >>= 1) x ^= __shfl_xor(x, d);
  return x;
}

// (the waves-per-SIMD choice is k_inflate's: the same decoder, the same chain of dependent round trips)
__global__ __launch_bounds__(kInflateThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_inflate_queue(
    const uint8_t* __restrict__ data, const ArchiveMember* __restrict__ members, const uint64_t* __restrict__ order, uint64_t n_order,
    unsigned long long* ticket, uint8_t* out, uint8_t* status, unsigned long long* err) {
  __shared__ __attribute__((aligned(8))) uint8_t table_mem[kWavesPerBlock][(inflate::kTableBytes + 7) & ~7u];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  inflate::Tables t;
  t.lens = table_mem[wave];
  t.lsym = reinterpret_cast<uint16_t*>(table_mem[wave] + inflate::kLensBytes);
  t.dsym = t.lsym + inflate::kLitSyms;
  t.work = t.dsym + inflate::kDistSyms;
  for (;;) {
    // The draw is made by ALL lanes in uniform control flow, lane 0 adding one and the others nothing (the compiler folds
    // them into one atomic per wave), and lane 0's old value is broadcast.  A draw under `if (lane == 0)` is not the same
    // thing: with the `if (lane == 0)` at the end of the body the compiler threads lane 0 from one to the other, the other
    // lanes reach the broadcast without lane 0 and read their own zero -- ticket 0 for ever.
    const unsigned long long drawn = atomicAdd(ticket, lane == 0 ? 1ull : 0ull);
    const uint64_t at = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)drawn) |
                        (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(drawn >> 32)) << 32;
    if (at >= n_order) break;                       // (every wave draws one ticket past the end, and no more)
    const uint64_t m = order[at];
    const ArchiveMember mem = members[m];
    WaveSink sink(out + mem.out_off, lane);
    uint32_t produced;
    const uint8_t r = inflate::inflate_member(data + mem.src_off, mem.src_len, mem.size, t, sink, &produced);
    if (lane == 0) {
      status[m] = r;
      if (r != inflate::kOk) atomicMin(err, (unsigned long long)m << 8 | r);
    }
  }
}

__global__ __launch_bounds__(kInflateThreads) void k_archive_chunks(const uint8_t* __restrict__ data, const ArchiveMember* __restrict__ members,
                                                                     const uint64_t* __restrict__ prefix, uint64_t n_members, uint64_t n_chunks,
                                                                     uint8_t* out, uint32_t* __restrict__ terms, int verify) {
  __shared__ uint32_t crc_table[256];
  for (uint32_t i = threadIdx.x; i < 256; i += kInflateThreads) crc_table[i] = inflate::crc_table_entry(i);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint64_t w = (uint64_t)blockIdx.x * kWavesPerBlock + wave; w < n_chunks; w += (uint64_t)gridDim.x * kWavesPerBlock) {
    const uint64_t m = archive::member_of_chunk(prefix, n_members, w);
    const ArchiveMember mem = members[m];
    const uint64_t c = w - prefix[m];
    const uint32_t lo = archive::chunk_begin(mem.size, c), n = archive::chunk_begin(mem.size, c + 1) - lo;
    const uint8_t* p;
    if (mem.inflated) {
      if (!verify) continue;
      p = out + mem.out_off + lo;
    } else {                                        // stored: the text is the entry's bytes; the CRC is taken from the source
      p = data + mem.src_off + lo;
      uint8_t* dst = out + mem.out_off + lo;
      for (uint32_t i = lane; i < n; i += 64) dst[i] = p[i];
      if (!verify) continue;
    }
    const uint32_t term = wave_xor(archive::chunk_lane_term(p, n, 64, lane, crc_table));
    if (lane == 0) terms[w] = term;
  }
}

__global__ __launch_bounds__(kInflateThreads) void k_archive_crc(const ArchiveMember* __restrict__ members, const uint64_t* __restrict__ prefix,
                                                                  uint64_t n_members, const uint32_t* __restrict__ terms, uint8_t* status,
                                                                  unsigned long long* err) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint64_t m = (uint64_t)blockIdx.x * kWavesPerBlock + wave; m < n_members; m += (uint64_t)gridDim.x * kWavesPerBlock) {
    if (status[m] != inflate::kOk) continue;        // (lane-uniform: one byte read by all)
    const ArchiveMember mem = members[m];
    const uint64_t first = prefix[m];
    const uint32_t x = wave_xor(archive::fold_lane_term(terms + first, prefix[m + 1] - first, mem.size, 64, lane));
    if (~x != mem.crc && lane == 0) {
      status[m] = inflate::kCrc;
      atomicMin(err, (unsigned long long)m << 8 | inflate::kCrc);
    }
  }
}

}  // namespace

void launch_inflate_queue(const uint8_t* data, const ArchiveMember* members, const uint64_t* order, uint64_t n_order, unsigned long long* ticket,
                          uint8_t* out, uint8_t* status, unsigned long long* err, Device& dev, hipStream_t s) {
  if (n_order == 0) return;
  hipLaunchKernelGGL(k_inflate_queue, dim3(grid_for(n_order, kWavesPerBlock, dev.grid_limit(), dev)), dim3(kInflateThreads), 0, s, data, members,
                     order, n_order, ticket, out, status, err);
  HIP_CHECK(hipGetLastError());
}

void launch_archive_chunks(const uint8_t* data, const ArchiveMember* members, const uint64_t* prefix, uint64_t n_members, uint64_t n_chunks,
                           uint8_t* out, uint32_t* terms, bool verify, Device& dev, hipStream_t s) {
  if (n_chunks == 0) return;
  hipLaunchKernelGGL(k_archive_chunks, dim3(grid_for(n_chunks, kWavesPerBlock, dev.grid_limit(), dev)), dim3(kInflateThreads), 0, s, data, members,
                     prefix, n_members, n_chunks, out, terms, verify ? 1 : 0);
  HIP_CHECK(hipGetLastError());
}

void launch_archive_crc(const ArchiveMember* members, const uint64_t* prefix, uint64_t n_members, const uint32_t* terms, uint8_t* status,
                        unsigned long long* err, Device& dev, hipStream_t s) {
  if (n_members == 0) return;
  hipLaunchKernelGGL(k_archive_crc, dim3(grid_for(n_members, kWavesPerBlock, dev.grid_limit(), dev)), dim3(kInflateThreads), 0, s, members, prefix,
                     n_members, terms, status, err);
  HIP_CHECK(hipGetLastError());
}

}  // namespace smh
