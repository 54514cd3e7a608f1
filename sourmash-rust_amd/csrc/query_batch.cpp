// query_batch.cpp -- what gather_many, search_many, lca_many and cluster share in front of their kernels (DESIGN.md 3.14,
// "Staging a batch"): the refusals of every query and of a CSR's offsets, the staging of a batch of sketches into one CSR in
// device memory, a chunk's relative offsets and the front half of a search chunk.
#include <algorithm>
#include <string>

#include "index.hpp"

namespace smh {

void ResidentIndex::check_queries(const char* op, const char* can, const KmerMinHash* const* queries, uint32_t nq) const {
  for (uint32_t q = 0; q < nq; q++) {
    const std::string who = std::string(op) + ": query " + std::to_string(q);
    if (queries[q]->num != 0) throw Error(kMsg, who + " is a num sketch; only scaled sketches (num == 0) " + can);
    if (any_num) throw Error(kMsg, who + ": the index holds a num sketch; only scaled sketches (num == 0) " + can);
    try {
      check_sketch(*queries[q]);
    } catch (const Error& e) {
      throw Error(e.code, who + ": " + e.message);
    }
  }
}

namespace {
[[noreturn]] void refuse_long_query(const char* who, uint64_t limit) {
  throw_internal(std::string(who) + ": a query of " + (limit == kQueryLimit31 ? "2^31" : "2^32 - 1") + " or more hashes");
}
}  // namespace

void check_query_offsets(const char* who, const uint64_t* qoff, uint32_t nq, uint64_t limit) {
  for (uint32_t q = 0; q < nq; q++) {
    if (qoff[q + 1] < qoff[q]) throw Error(kMsg, std::string(who) + ": offsets must ascend (query " + std::to_string(q) + ")");
    if (qoff[q + 1] - qoff[q] >= limit) refuse_long_query(who, limit);
  }
}

QueryBatch::QueryBatch(const KmerMinHash* const* queries, uint32_t nq, const char* who, uint64_t limit, bool want_abunds, Device& dev)
    : ws(dev.stream()), qoff((size_t)nq + 1, 0) {
  hipStream_t s = dev.stream();
  bool any_dev = false;
  uint64_t host_total = 0;
  for (uint32_t q = 0; q < nq; q++) {
    const KmerMinHash& Q = *queries[q];
    Q.flush_pending();
    const uint64_t lq = Q.dev ? Q.dev->n : Q.mins.size();
    if (want_abunds && !Q.dev && Q.has_abunds && Q.abunds.size() != lq)
      throw_internal(std::string(who) + ": the abundance vector of query " + std::to_string(q) + " does not match its hashes (quirks Q5/Q6)");
    if (want_abunds && Q.dev && Q.has_abunds && !Q.dev->has_counts && !Q.dev->has_runs)
      throw_internal(std::string(who) + ": the device state of query " + std::to_string(q) + " carries no abundances");
    if (lq >= limit) refuse_long_query(who, limit);
    qoff[q + 1] = qoff[q] + lq;
    with_abunds |= want_abunds && Q.has_abunds;
    any_dev |= Q.dev != nullptr;
    if (!Q.dev) host_total += lq;
  }
  const uint64_t total = qoff[nq];
  const size_t words = with_abunds ? 2 : 1;
  csr = ws.take<uint64_t>(total * words);
  uint64_t* d_h = csr;
  uint64_t* d_a = d_h + total;   // (read only when with_abunds)
  // the host states, one layout for both routes: [the hashes of each | the abundances of each], one query after another
  std::vector<uint64_t> stage(host_total * words);
  uint64_t at = 0;
  for (uint32_t q = 0; q < nq; q++) {
    const KmerMinHash& Q = *queries[q];
    if (Q.dev) continue;
    std::copy(Q.mins.begin(), Q.mins.end(), stage.begin() + at);
    if (with_abunds && Q.has_abunds) std::copy(Q.abunds.begin(), Q.abunds.end(), stage.begin() + host_total + at);
    else if (with_abunds) std::fill_n(stage.begin() + host_total + at, Q.mins.size(), 1ull);
    at += Q.mins.size();
  }
  if (!any_dev) {   // straight into place: the host states are the CSR
    if (!stage.empty()) HIP_CHECK(hipMemcpyAsync(d_h, stage.data(), stage.size() * 8, hipMemcpyHostToDevice, s));
  } else {
    uint64_t* u_h = ws.take<uint64_t>(stage.size());
    if (!stage.empty()) HIP_CHECK(hipMemcpyAsync(u_h, stage.data(), stage.size() * 8, hipMemcpyHostToDevice, s));
    at = 0;
    for (uint32_t q = 0; q < nq; q++) {
      const KmerMinHash& Q = *queries[q];
      const uint64_t lq = qoff[q + 1] - qoff[q];
      if (lq == 0) continue;
      if (!Q.dev) {
        HIP_CHECK(hipMemcpyAsync(d_h + qoff[q], u_h + at, lq * 8, hipMemcpyDeviceToDevice, s));
        if (with_abunds) HIP_CHECK(hipMemcpyAsync(d_a + qoff[q], u_h + host_total + at, lq * 8, hipMemcpyDeviceToDevice, s));
        at += lq;
        continue;
      }
      const DeviceSketch& S = *Q.dev;
      HIP_CHECK(hipMemcpyAsync(d_h + qoff[q], S.uniq.ptr, lq * 8, hipMemcpyDeviceToDevice, s));
      if (!with_abunds) continue;
      if (Q.has_abunds && S.has_counts) HIP_CHECK(hipMemcpyAsync(d_a + qoff[q], S.counts.ptr, lq * 8, hipMemcpyDeviceToDevice, s));
      else launch_gather_many_weights(Q.has_abunds ? S.starts.as<uint32_t>() : nullptr, (uint32_t)S.total, (uint32_t)lq, d_a + qoff[q], s);
    }
  }
  HIP_CHECK(hipStreamSynchronize(s));   // (`stage` is read by the upload)
}

size_t append_chunk_offsets(const uint64_t* qoff, uint32_t a, uint32_t b, std::vector<uint32_t>* rel) {
  const size_t at = rel->size();
  for (uint32_t k = a; k <= b; k++) rel->push_back((uint32_t)(qoff[k] - qoff[a]));
  return at;
}

void upload_chunk_offsets(const uint64_t* qoff, uint32_t a, uint32_t b, std::vector<uint32_t>* rel, uint32_t* dst, hipStream_t s) {
  rel->clear();
  append_chunk_offsets(qoff, a, b, rel);
  HIP_CHECK(hipMemcpyAsync(dst, rel->data(), rel->size() * 4, hipMemcpyHostToDevice, s));
}

SearchChunk ResidentIndex::search_chunk(const uint64_t* qh, const uint64_t* qoff, uint32_t a, uint32_t b, uint32_t metric, double threshold,
                                        uint32_t threshold_common, uint32_t self) const {
  SearchChunk ck;
  ck.hashes = qh + qoff[a];
  ck.nq = b - a; ck.T = (uint32_t)(qoff[b] - qoff[a]); ck.n = n;
  ck.q0 = self ? a : 0;
  ck.tiles = (n + kSearchTile - 1) / kSearchTile;
  ck.node_offsets = offsets.as<uint64_t>();
  ck.metric = metric; ck.self = self; ck.threshold_common = threshold_common; ck.threshold = threshold;
  return ck;
}

uint32_t search_chunk_rows(const MatchDirectory& dir, const SearchChunk& ck, Device& dev, hipStream_t s) {
  HIP_CHECK(hipMemsetAsync(ck.c, 0, (size_t)ck.nq * ck.n * 4, s));
  launch_search_many_probe(dir, ck, dev, s);
  launch_search_many_select(ck, dev, s);
  uint32_t R = 0;
  HIP_CHECK(hipMemcpyAsync(&R, ck.tile_rows + (size_t)ck.nq * ck.tiles, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return R;
}

}  // namespace smh
