// nearest.cpp -- ResidentIndex::nearest_many / nearest_dev / nearest_self (the rules are in
// include/sourmash_amd.h, smh_index_nearest_many): search_many's chunks, and per chunk its front half (the probe and the
// select), then the clamp, the one read-back that sizes the candidates and the rows, the tile sort and the merge.  The kernels
// are in nearest_kernels.hip; the checks and the staging of the queries are query_batch.cpp's.
#include <algorithm>
#include <string>

#include "index.hpp"

namespace smh {

void check_nearest_k(uint32_t k) {
  if (k == 0) throw Error(kMsg, "nearest_many: k is 0; it must be 1 .. " + std::to_string(kNearestMaxK));
  if (k > kNearestMaxK) throw Error(kMsg, "nearest_many: k is " + std::to_string(k) + "; the largest k is " + std::to_string(kNearestMaxK));
}

SearchRow* ResidentIndex::nearest_dev(const uint64_t* qh, const uint64_t* qoff, uint32_t nq, uint32_t k, uint32_t metric, double threshold,
                                      uint32_t threshold_common, uint32_t self, uint64_t* row_offsets, Device& dev, hipStream_t s) {
  check_search(metric, threshold);   // (search_chunks' first check again: the refusal of k comes behind it)
  check_nearest_k(k);
  std::vector<uint32_t> row_at;
  auto tail = [&](const MatchDirectory& dir, const SearchChunk& ck, Workspace& ws, SearchRowsOut& out, uint32_t* starts) -> uint32_t {
    const uint32_t Qc = ck.nq;
    const size_t cells = (size_t)Qc * ck.tiles;
    NearestChunk nc;
    nc.k = k;
    nc.cand_at = ws.take<uint32_t>(cells + 1 + Qc + 1);
    nc.row_at = nc.cand_at + cells + 1;
    HIP_CHECK(hipMemsetAsync(ck.c, 0, (size_t)Qc * n * 4, s));
    launch_search_many_probe(dir, ck, dev, s);
    launch_search_many_select(ck, dev, s);
    launch_nearest_clamp(ck, nc, dev, s);
    uint32_t sized[2] = {0, 0};   // the chunk's candidates, and candidates + rows (one scan runs over cand_at and row_at)
    HIP_CHECK(hipMemcpyAsync(&sized[0], nc.cand_at + cells, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&sized[1], nc.row_at + Qc, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const uint32_t C = sized[0], R = sized[1] - sized[0];
    if (R == 0) return 0;
    SearchRow* dst = out.room(R);   // (before the device rows: a refusal leaves only blocks that go back by themselves)
    nc.cand_v = reinterpret_cast<uint64_t*>(ws.take<uint8_t>((size_t)C * 12));   // C u64 values, then C u32 nodes
    nc.cand_n = reinterpret_cast<uint32_t*>(nc.cand_v + C);
    SearchRow* d_rows = ws.take<SearchRow>(R);
    launch_nearest_tile(ck, nc, dev, s);
    launch_nearest_merge(ck, nc, d_rows, dev, s);
    row_at.resize((size_t)Qc + 1);
    HIP_CHECK(hipMemcpyAsync(dst, d_rows, (size_t)R * sizeof(SearchRow), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(row_at.data(), nc.row_at, ((size_t)Qc + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (uint32_t j = 1; j < Qc; j++) starts[j] = row_at[j] - row_at[0];
    return R;
  };
  return search_chunks("nearest_many", "nearest_chunk", qh, qoff, nq, metric, threshold, threshold_common, self, row_offsets, dev, s, tail);
}

SearchRow* ResidentIndex::nearest_many(const KmerMinHash* const* queries, uint32_t nq, uint32_t k, uint32_t metric, double threshold,
                                       uint32_t threshold_common, uint64_t* row_offsets, Device& dev) {
  check_search(metric, threshold);
  check_nearest_k(k);
  check_queries("nearest_many", "can be searched", queries, nq);
  check_directory_size("nearest_many");
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  const QueryBatch batch(queries, nq, "nearest_many", kQueryLimit32, false, dev);
  return nearest_dev(batch.hashes(), batch.offsets(), nq, k, metric, threshold, threshold_common, kSearchNotSelf, row_offsets, dev, dev.stream());
}

SearchRow* ResidentIndex::nearest_self(uint32_t k, uint32_t metric, double threshold, uint32_t threshold_common, uint64_t* row_offsets,
                                       Device& dev) {
  check_search(metric, threshold);
  check_nearest_k(k);
  if (any_num) throw Error(kMsg, "nearest_self: the index holds a num sketch; only scaled sketches (num == 0) can be searched");
  check_index(*this);   // nodes that differ refuse each other (O(1) when they agree)
  check_directory_size("nearest_many");
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  // the queries are the nodes where they lie: the resident CSR and its offsets
  return nearest_dev(hashes.as<uint64_t>(), h_offsets.data(), n, k, metric, threshold, threshold_common, kSearchNoDiagonal, row_offsets, dev,
                     dev.stream());
}

}  // namespace smh
