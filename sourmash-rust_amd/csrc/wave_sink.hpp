// wave_sink.hpp -- the sink of the device decoders (inflate_kernels.hip, archive_kernels.hip): where one wave that runs
// inflate_core.hpp lane-uniform puts a member's bytes.  Literal runs are kept one byte per lane and stored together, a match
// copy or a stored block is spread over the lanes.
//
// Cross-lane read-after-write: a copy reads bytes of the member's output slice -- the window is the slice itself, in global
// memory -- that OTHER lanes of this wave stored in an earlier step.  The sink puts a workgroup-scope release fence behind
// its stores and an acquire fence in front of the loads of every copy.  Inside one copy no lane reads a byte the same copy
// writes: a distance below the length is expanded as the periodic pattern it is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smh {

struct WaveSink {
  uint8_t* out;        // the member's slice
  uint32_t lane;
  uint32_t nlit = 0;   // literals not stored yet: out[lit_pos + i] is lane i's `mine`
  uint32_t lit_pos = 0;
  uint8_t mine = 0;
  __device__ WaveSink(uint8_t* o, uint32_t l) : out(o), lane(l) {}
  __device__ void flush() {
    if (nlit) {
      if (lane < nlit) out[lit_pos + lane] = mine;
      nlit = 0;
    }
  }
  __device__ void lit(uint32_t pos, uint8_t b) {
    if (nlit == 0) lit_pos = pos;
    if (lane == nlit) mine = b;
    if (++nlit == 64) flush();
  }
  // orders the loads that follow behind the stores every lane of the wave has issued
  __device__ static void publish() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  __device__ void copy(uint32_t pos, uint32_t dist, uint32_t len) {
    flush();
    publish();
    const uint8_t* src = out + (pos - dist);
    if (dist >= len) {
      for (uint32_t i = lane; i < len; i += 64) out[pos + i] = src[i];
    } else {
      for (uint32_t i = lane; i < len; i += 64) out[pos + i] = src[i % dist];
    }
  }
  __device__ void stored(uint32_t pos, const uint8_t* src, uint32_t n) {
    flush();
    for (uint32_t i = lane; i < n; i += 64) out[pos + i] = src[i];
  }
};

}  // namespace smh
