// sketch_launch.hpp -- host code shared by the launchers of the sketch kernels (sketch_kernels.hip,
// sketch_dna_kernels.hip, sketch_protein_kernels.hip, sketch_amino_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device.hpp"
#include "kernels.hpp"

namespace smh {

inline int sketch_grid(uint64_t items, int per_block, int cap) {
  uint64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > (uint64_t)cap) g = cap;
  return (int)g;
}

// Workgroups of `kernel` that the chip holds at once: what the runtime's occupancy query says fits one CU with `threads`
// lanes and `lds` bytes of dynamic LDS (registers and static LDS are the kernel's own), times the CUs.  More workgroups
// than that run in rounds; exactly that many, taking their tiles dynamically, keep every CU busy to the last tile.  Asked
// once per kernel and LDS size, on the host.
template <class Kernel>
static uint64_t resident_workgroups(Kernel kernel, int threads, size_t lds, Device& dev) {
  static std::mutex mu;
  static std::map<std::pair<const void*, size_t>, int> cache;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_pair(reinterpret_cast<const void*>(kernel), lds);
  auto it = cache.find(key);
  if (it == cache.end()) {
    int per_cu = 0;
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds));
    if (per_cu < 1) throw_internal("a sketch kernel does not fit a compute unit (occupancy query)");
    it = cache.emplace(key, per_cu).first;
  }
  return (uint64_t)it->second * (uint64_t)dev.cu_count();
}

// the batch with its per-tile record table (k_tile_records) for a launch of `ntiles` tiles from position `base`
// (k_tile_records and the definition: sketch_kernels.hip; hidden: the library's exported symbols stay what they were)
__attribute__((visibility("hidden"))) SeqBatch with_tile_records(const SeqBatch& b, uint32_t min_len, uint64_t base, uint64_t tile, uint64_t ntiles, Device& dev,
                           hipStream_t s);

}  // namespace smh
