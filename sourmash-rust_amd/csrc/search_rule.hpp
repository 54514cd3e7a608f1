// search_rule.hpp -- the rule of the thresholded search on one (query, node) pair and the pass of a workgroup over one tile of
// a query's counters (include/sourmash_amd.h, smh_index_search_many), shared by search_many_kernels.hip,
// cluster_kernels.hip and nearest_kernels.hip: clustering's adjacency and a query's neighbours ARE this rule, through this
// device function.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace smh {
namespace {

constexpr uint32_t kTileThreads = 256;
constexpr uint32_t kSteps = kSearchTile / kTileThreads;   // nodes per thread
static_assert(kSearchTile == kTileThreads * kSteps && kTileThreads % 64 == 0, "a wave takes whole steps of 64 nodes");

struct Rule {
  const uint64_t* __restrict__ node_offsets;
  double threshold;
  uint32_t metric, self, threshold_common;
};

// the metric's value of a pair with common >= 1: the ONE division of the header (the thresholded search compares it, the
// nearest-neighbour kernels order by its bit pattern)
__device__ __forceinline__ double metric_value(const Rule& r, uint32_t common, uint32_t lq, uint32_t ls) {
  uint64_t den;
  switch (r.metric) {
    case kSearchJaccard: den = (uint64_t)lq + ls - common; break;   // (>= 1: common >= 1)
    case kSearchContainmentNode: den = ls; break;
    case kSearchContainmentQuery: den = lq; break;
    default: den = lq < ls ? lq : ls; break;
  }
  return (double)common / (double)den;
}

// the rule of the header on one pair: node i (of size ls) and the query that is node `me` in the self modes (of size lq)
__device__ __forceinline__ bool survives(const Rule& r, uint32_t common, uint32_t lq, uint32_t ls, uint32_t i, uint32_t me) {
  if (common < r.threshold_common) return false;   // (threshold_common >= 1: a pair that shares nothing ends here)
  if (r.self == kSearchNoDiagonal && i == me) return false;
  if (r.self == kSearchUpperOnly && i <= me) return false;
  return metric_value(r, common, lq, ls) > r.threshold;
}

// What a thread finds at its kSteps nodes of tile blockIdx.x of query blockIdx.y: common[k], size[k] and bit k of the
// returned mask for a survivor.  Step k of wave w looks at node tile * kSearchTile + w * 64 * kSteps + k * 64 + lane.
__device__ __forceinline__ uint32_t scan_tile(const Rule& r, const uint32_t* __restrict__ c, const uint32_t* __restrict__ qoff, uint32_t n,
                                              uint32_t q0, uint32_t* lq_out, uint32_t* first, uint32_t common[kSteps], uint32_t size[kSteps]) {
  const uint32_t q = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t lq = qoff[q + 1] - qoff[q];
  const uint32_t i0 = blockIdx.x * kSearchTile + wave * 64 * kSteps + lane;
  const uint32_t* __restrict__ cq = c + (size_t)q * n;
  uint32_t mask = 0;
#pragma unroll
  for (uint32_t k = 0; k < kSteps; k++) {
    const uint32_t i = i0 + k * 64;
    common[k] = 0; size[k] = 0;
    if (i < n) {
      common[k] = cq[i];
      if (common[k]) {   // (most pairs share nothing: their sizes are not read)
        size[k] = (uint32_t)(r.node_offsets[i + 1] - r.node_offsets[i]);
        if (survives(r, common[k], lq, size[k], i, q0 + q)) mask |= 1u << k;
      }
    }
  }
  *lq_out = lq;
  *first = i0;
  return mask;
}

}  // namespace
}  // namespace smh
