// inflate_kernels.hip -- blocked gzip inflated on the device: one wave per member, members walked in a
// gridDim-stride loop.  The decoder is inflate_core.hpp, run lane-uniform: all 64 lanes read the same payload bytes, hold the
// same bit buffer and counters and write the same values to the wave's tables in LDS (identical stores to one address; every
// lane reads back what it has itself written, so the tables need no cross-lane ordering).  The lanes differ only in the sink
// (wave_sink.hpp, shared with archive_kernels.hip):
// literal runs are kept one byte per lane and stored together, a match copy or a stored block is spread over the lanes.
//
// Cross-lane read-after-write: a copy reads bytes of the member's output slice -- the window is the slice itself, in global
// memory -- that OTHER lanes of this wave stored in an earlier step.  The sink puts a workgroup-scope release fence behind
// its stores and an acquire fence in front of the loads of every copy, and of the CRC pass.  Inside one copy no lane reads a
// byte the same copy writes: a distance below the length is expanded as the periodic pattern it is.
#include "inflate_core.hpp"
#include "kernels.hpp"
#include "wave_sink.hpp"

namespace smh {

namespace {

constexpr uint32_t kWavesPerBlock = kInflateThreads / 64;

// The decode is a chain of dependent round trips, so waves in flight are what it runs on: four per SIMD (128 VGPRs, two
// spilled) measured 19 % faster than the three the compiler takes by itself at 144.
__global__ __launch_bounds__(kInflateThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_inflate(const uint8_t* __restrict__ data, const InflateMember* __restrict__ members,
                                                             uint64_t n_members, uint8_t* out, int verify_crc, uint8_t* status,
                                                             unsigned long long* err) {
  __shared__ uint32_t crc_table[256];
  __shared__ __attribute__((aligned(8))) uint8_t table_mem[kWavesPerBlock][(inflate::kTableBytes + 7) & ~7u];
  for (uint32_t i = threadIdx.x; i < 256; i += kInflateThreads) crc_table[i] = inflate::crc_table_entry(i);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  inflate::Tables t;
  t.lens = table_mem[wave];
  t.lsym = reinterpret_cast<uint16_t*>(table_mem[wave] + inflate::kLensBytes);
  t.dsym = t.lsym + inflate::kLitSyms;
  t.work = t.dsym + inflate::kDistSyms;
  for (uint64_t m = (uint64_t)blockIdx.x * kWavesPerBlock + wave; m < n_members; m += (uint64_t)gridDim.x * kWavesPerBlock) {
    const InflateMember mem = members[m];
    uint8_t* dst = out + mem.out_off;
    WaveSink sink(dst, lane);
    uint32_t produced;
    uint8_t r = inflate::inflate_member(data + mem.payload_off, mem.payload_len, mem.isize, t, sink, &produced);
    if (r == inflate::kOk && verify_crc) {
      WaveSink::publish();
      uint32_t term = inflate::crc_lane_term(dst, mem.isize, 64, lane, crc_table);
      for (int d = 32; d; d >>= 1) term ^= __shfl_xor(term, d);
      if (~term != mem.crc) r = inflate::kCrc;
    }
    if (lane == 0) {
      status[m] = r;
      if (r != inflate::kOk) atomicMin(err, (unsigned long long)m << 8 | r);
    }
  }
}

}  // namespace

void launch_inflate(const uint8_t* data, const InflateMember* members, uint64_t n_members, uint8_t* out, bool verify_crc, uint8_t* status,
                    unsigned long long* err, Device& dev, hipStream_t s) {
  if (n_members == 0) return;
  hipLaunchKernelGGL(k_inflate, dim3(grid_for(n_members, kWavesPerBlock, dev.grid_limit(), dev)), dim3(kInflateThreads), 0, s, data, members,
                     n_members, out, verify_crc ? 1 : 0, status, err);
  HIP_CHECK(hipGetLastError());
}

}  // namespace smh
