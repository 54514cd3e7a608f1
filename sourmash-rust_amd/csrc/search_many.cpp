// search_many.cpp -- ResidentIndex::search_many / search_self (the rules are in include/sourmash_amd.h,
// smh_index_search_many): the chunks cut at query boundaries, and per chunk the emit and the rows' way into the caller's
// array.  The checks of every query, the staging of a batch of sketches into one CSR in device memory and a chunk's front half
// (the probe, the select, the sizing read-back) are query_batch.cpp's.  The kernels are in search_many_kernels.hip; the hash
// directory is the index's (index.cpp), shared with match, gather_many and the LCA.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "index.hpp"

namespace smh {

uint64_t g_search_many_budget = kSearchManyBudget;

uint32_t search_many_chunk_end(const uint64_t* qoff, uint32_t a, uint32_t nq, uint32_t n_nodes, uint64_t budget) {
  return query_chunk_end(qoff, a, nq, n_nodes, budget, kSearchMaxQueries);
}

void check_search(uint32_t metric, double threshold) {
  if (std::isnan(threshold)) throw Error(kMsg, "search_many: the threshold is NaN");
  if (metric > kSearchMaxContainment) throw Error(kMsg, "search_many: unknown metric " + std::to_string(metric));
}

SearchRow* SearchRowsOut::room(size_t more) {
  if (len + more > cap || !p) {
    const size_t want = std::max<size_t>({len + more, cap * 2, 1});
    SearchRow* np = (SearchRow*)realloc(p, want * sizeof(SearchRow));
    if (!np) throw Error(kMsg, std::string(who) + ": out of memory for " + std::to_string(want) + " rows");
    p = np; cap = want;
  }
  return p + len;
}

SearchRow* ResidentIndex::search_chunks(const char* who, const char* chunk_counter, const uint64_t* qh, const uint64_t* qoff, uint32_t nq,
                                        uint32_t metric, double threshold, uint32_t threshold_common, uint32_t self, uint64_t* row_offsets,
                                        Device& dev, hipStream_t s, const SearchChunkTail& tail) {
  const std::string name(who);
  check_search(metric, threshold);
  if (any_num) throw Error(kMsg, name + ": the index holds a num sketch; only scaled sketches (num == 0) can be searched");
  if (threshold_common == 0) threshold_common = 1;
  check_query_offsets(who, qoff, nq, kQueryLimit32);
  check_directory_size(who);
  if (n > 0xffffffffu - 2 * kSearchTile) throw_internal(name + ": too many nodes");
  const uint64_t total = nq ? qoff[nq] - qoff[0] : 0;
  std::vector<uint64_t> roff((size_t)nq + 1, 0);
  SearchRowsOut out(who);
  auto finish = [&] {
    SearchRow* r = out.release();   // (may refuse: nothing has been written then)
    std::copy(roff.begin(), roff.end(), row_offsets);
    return r;
  };
  if (n == 0 || total == 0) return finish();

  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  const MatchDirectory dir = ensure_directory(who, dev, s);
  if (dir.n_hashes == 0) return finish();
  std::vector<uint32_t> rel, starts;
  const uint32_t tiles = (n + kSearchTile - 1) / kSearchTile;

  for (uint32_t a = 0, b = 0; a < nq; a = b) {
    b = search_many_chunk_end(qoff, a, nq, n, g_search_many_budget);
    const uint32_t Qc = b - a;
    const uint64_t T = qoff[b] - qoff[a];
    const uint64_t base = roff[a];
    for (uint32_t q = a; q < b; q++) roff[q + 1] = base;
    dev.count(chunk_counter);
    if (T == 0) continue;
    Workspace ws(s);
    SearchChunk ck = search_chunk(qh, qoff, a, b, metric, threshold, threshold_common, self);
    uint32_t* d_qoff = ws.take<uint32_t>((size_t)Qc + 1);
    ck.qoff = d_qoff;
    ck.c = ws.take<uint32_t>((size_t)Qc * n);
    ck.tile_rows = ws.take<uint32_t>((size_t)Qc * tiles + 1);
    upload_chunk_offsets(qoff, a, b, &rel, d_qoff, s);
    starts.assign(Qc, 0);
    const uint32_t R = tail(dir, ck, ws, out, starts.data());
    out.len += R;
    for (uint32_t k = 1; k < Qc; k++) roff[a + k] = base + starts[k];
    roff[b] = base + R;
  }
  return finish();
}

SearchRow* ResidentIndex::search_many_dev(const uint64_t* qh, const uint64_t* qoff, uint32_t nq, uint32_t metric, double threshold,
                                          uint32_t threshold_common, uint32_t self, uint64_t* row_offsets, Device& dev, hipStream_t s) {
  auto tail = [&](const MatchDirectory& dir, const SearchChunk& ck, Workspace& ws, SearchRowsOut& out, uint32_t* starts) -> uint32_t {
    uint32_t* d_qrows = ws.take<uint32_t>(ck.nq);
    const uint32_t R = search_chunk_rows(dir, ck, dev, s);
    if (R == 0) return 0;
    SearchRow* dst = out.room(R);   // (before the device rows: a refusal leaves only blocks that go back by themselves)
    SearchRow* d_rows = ws.take<SearchRow>(R);
    launch_search_many_emit(ck, d_rows, d_qrows, dev, s);
    HIP_CHECK(hipMemcpyAsync(dst, d_rows, (size_t)R * sizeof(SearchRow), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(starts, d_qrows, (size_t)ck.nq * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return R;
  };
  return search_chunks("search_many", "search_many_chunk", qh, qoff, nq, metric, threshold, threshold_common, self, row_offsets, dev, s, tail);
}

SearchRow* ResidentIndex::search_many(const KmerMinHash* const* queries, uint32_t nq, uint32_t metric, double threshold,
                                      uint32_t threshold_common, uint64_t* row_offsets, Device& dev) {
  check_search(metric, threshold);
  check_queries("search_many", "can be searched", queries, nq);
  check_directory_size("search_many");
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  const QueryBatch batch(queries, nq, "search_many", kQueryLimit32, false, dev);
  return search_many_dev(batch.hashes(), batch.offsets(), nq, metric, threshold, threshold_common, kSearchNotSelf, row_offsets, dev, dev.stream());
}

SearchRow* ResidentIndex::search_self(uint32_t metric, double threshold, uint32_t threshold_common, bool upper_only, uint64_t* row_offsets,
                                      Device& dev) {
  check_search(metric, threshold);
  if (any_num) throw Error(kMsg, "search_self: the index holds a num sketch; only scaled sketches (num == 0) can be searched");
  check_index(*this);   // nodes that differ refuse each other (O(1) when they agree)
  check_directory_size("search_many");
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  // the queries are the nodes where they lie: the resident CSR and its offsets
  return search_many_dev(hashes.as<uint64_t>(), h_offsets.data(), n, metric, threshold, threshold_common,
                         upper_only ? kSearchUpperOnly : kSearchNoDiagonal, row_offsets, dev, dev.stream());
}

}  // namespace smh
