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
  check_search(metric, threshold);
  check_nearest_k(k);
  if (any_num) throw Error(kMsg, "nearest_many: the index holds a num sketch; only scaled sketches (num == 0) can be searched");
  if (threshold_common == 0) threshold_common = 1;
  check_query_offsets("nearest_many", qoff, nq, kQueryLimit32);
  check_directory_size("nearest_many");
  if (n > 0xffffffffu - 2 * kSearchTile) throw_internal("nearest_many: too many nodes");
  const uint64_t total = nq ? qoff[nq] - qoff[0] : 0;
  std::vector<uint64_t> roff((size_t)nq + 1, 0);
  SearchRowsOut out("nearest_many");
  auto finish = [&] {
    SearchRow* r = out.release();   // (may refuse: nothing has been written then)
    std::copy(roff.begin(), roff.end(), row_offsets);
    return r;
  };
  if (n == 0 || total == 0) return finish();

  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  const MatchDirectory dir = ensure_directory("nearest_many", dev, s);
  if (dir.n_hashes == 0) return finish();
  std::vector<uint32_t> rel, qrows;
  const uint32_t tiles = (n + kSearchTile - 1) / kSearchTile;

  for (uint32_t a = 0, b = 0; a < nq; a = b) {
    b = search_many_chunk_end(qoff, a, nq, n, g_search_many_budget);
    const uint32_t Qc = b - a;
    const uint64_t T = qoff[b] - qoff[a];
    const uint64_t base = roff[a];
    for (uint32_t q = a; q < b; q++) roff[q + 1] = base;
    dev.count("nearest_chunk");
    if (T == 0) continue;
    const size_t cells = (size_t)Qc * tiles;
    PoolBlock d_qoff(((size_t)Qc + 1) * 4), d_c((size_t)Qc * n * 4), d_tiles((cells + 1) * 4), d_at((cells + 1 + Qc + 1) * 4);
    SearchChunk ck = search_chunk(qh, qoff, a, b, metric, threshold, threshold_common, self);
    ck.qoff = d_qoff.as<uint32_t>();
    ck.c = d_c.as<uint32_t>();
    ck.tile_rows = d_tiles.as<uint32_t>();
    NearestChunk nc;
    nc.k = k;
    nc.cand_at = d_at.as<uint32_t>();
    nc.row_at = nc.cand_at + cells + 1;
    upload_chunk_offsets(qoff, a, b, &rel, d_qoff.as<uint32_t>(), s);
    HIP_CHECK(hipMemsetAsync(ck.c, 0, (size_t)Qc * n * 4, s));
    launch_search_many_probe(dir, ck, dev, s);
    launch_search_many_select(ck, dev, s);
    launch_nearest_clamp(ck, nc, dev, s);
    uint32_t sized[2] = {0, 0};   // the chunk's candidates, and candidates + rows (one scan runs over cand_at and row_at)
    HIP_CHECK(hipMemcpyAsync(&sized[0], nc.cand_at + cells, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&sized[1], nc.row_at + Qc, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    d_qoff.synced = d_c.synced = d_tiles.synced = d_at.synced = true;
    const uint32_t C = sized[0], R = sized[1] - sized[0];
    if (R == 0) continue;
    SearchRow* dst = out.room(R);   // (before the device rows: a refusal leaves only blocks that go back by themselves)
    PoolBlock d_cand((size_t)C * 12), d_rows((size_t)R * sizeof(SearchRow));
    nc.cand_v = d_cand.as<uint64_t>();
    nc.cand_n = reinterpret_cast<uint32_t*>(nc.cand_v + C);
    launch_nearest_tile(ck, nc, dev, s);
    launch_nearest_merge(ck, nc, d_rows.as<SearchRow>(), dev, s);
    qrows.resize((size_t)Qc + 1);
    HIP_CHECK(hipMemcpyAsync(dst, d_rows.ptr, (size_t)R * sizeof(SearchRow), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(qrows.data(), nc.row_at, ((size_t)Qc + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    d_cand.synced = d_rows.synced = true;
    out.len += R;
    for (uint32_t j = 1; j <= Qc; j++) roff[a + j] = base + (qrows[j] - qrows[0]);
  }
  return finish();
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
