// cluster.cpp -- ResidentIndex::cluster (the rules are in include/sourmash_amd.h, smh_index_cluster): the
// checks, the chunks of queries (search_self's cutter and budget), and per linkage the launches of cluster_kernels.hip and of
// the search kernels.  Nothing proportional to the pairs comes to the host: one copy of 8 (greedy with rep_common: 12) bytes
// per node does.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>

#include "index.hpp"

namespace smh {

uint64_t g_cluster_pair_budget = kClusterPairBudget;
uint32_t g_cluster_rounds = kClusterRoundsPerSync;

void check_cluster(uint32_t metric, double threshold, uint32_t linkage, bool want_rep_common) {
  if (std::isnan(threshold)) throw Error(kMsg, "cluster: the threshold is NaN");
  if (metric > kSearchMaxContainment) throw Error(kMsg, "cluster: unknown metric " + std::to_string(metric));
  if (metric != kSearchJaccard && metric != kSearchMaxContainment)
    throw Error(kMsg, "cluster: metric " + std::to_string(metric) + " is directed; clustering takes the symmetric ones (jaccard, "
                      "max_containment: either direction exceeding the threshold is what max_containment says)");
  if (linkage > kClusterGreedy) throw Error(kMsg, "cluster: unknown linkage " + std::to_string(linkage));
  if (want_rep_common && linkage != kClusterGreedy) throw Error(kMsg, "cluster: rep_common is defined for the greedy linkage only");
}

namespace {
struct Chunk { uint32_t a, b; size_t rel_at; };   // queries [a, b); where its relative offsets start in the uploaded array
}

void ResidentIndex::cluster(uint32_t metric, double threshold, uint32_t threshold_common, uint32_t linkage, const uint32_t* scores,
                            uint32_t* cluster_out, uint32_t* representative, uint32_t* rep_common, uint32_t* n_clusters, Device& dev) {
  check_cluster(metric, threshold, linkage, rep_common != nullptr);
  if (any_num) throw Error(kMsg, "cluster: the index holds a num sketch; only scaled sketches (num == 0) can be clustered");
  check_index(*this);   // nodes that differ refuse each other (O(1) when they agree)
  check_directory_size("cluster");
  if (n > 0xffffffffu - 2 * kSearchTile) throw_internal("cluster: too many nodes");
  if (threshold_common == 0) threshold_common = 1;
  if (n == 0) { *n_clusters = 0; return; }
  const uint64_t* qoff = h_offsets.data();
  const bool greedy = linkage == kClusterGreedy;
  if (qoff[n] == qoff[0]) {   // every sketch is empty: nothing is adjacent to anything
    for (uint32_t v = 0; v < n; v++) { cluster_out[v] = v; representative[v] = v; if (rep_common) rep_common[v] = 0; }
    *n_clusters = n;
    return;
  }

  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  const MatchDirectory dir = ensure_directory("cluster", dev, s);
  const uint32_t tiles = (n + kSearchTile - 1) / kSearchTile;

  // every chunk's relative offsets, prepared once and uploaded once (a vector reused per chunk would be rewritten under an
  // asynchronous copy that still reads it)
  std::vector<Chunk> chunks;
  std::vector<uint32_t> rel;
  uint32_t max_q = 0;
  for (uint32_t a = 0, b = 0; a < n; a = b) {
    b = search_many_chunk_end(qoff, a, n, n, g_search_many_budget);
    chunks.push_back({a, b, append_chunk_offsets(qoff, a, b, &rel)});
    max_q = std::max(max_q, b - a);
  }
  const size_t out_words = (size_t)n * (greedy ? 3 : 2) + 1;
  std::vector<uint32_t> host_out(out_words), order, rank;   // (what copies on the stream touch is declared ahead of the workspace, which waits)
  // the blocks of the whole call: they go back when it ends, on every way out, behind a wait for the stream
  Workspace ws(s);
  uint32_t* d_rel = ws.take<uint32_t>(rel.size());
  uint32_t* d_c = ws.take<uint32_t>((size_t)max_q * n);
  uint32_t* d_out = ws.take<uint32_t>(out_words);
  uint32_t* d_scores = reinterpret_cast<uint32_t*>(ws.take<uint8_t>(scores && !greedy ? (size_t)n * 4 : 1));   // (greedy ranks the nodes on the host)
  HIP_CHECK(hipMemcpyAsync(d_rel, rel.data(), rel.size() * 4, hipMemcpyHostToDevice, s));
  if (scores && !greedy) HIP_CHECK(hipMemcpyAsync(d_scores, scores, (size_t)n * 4, hipMemcpyHostToDevice, s));
  auto chunk_of = [&](const Chunk& c) {
    SearchChunk ck = search_chunk(hashes.as<uint64_t>(), qoff, c.a, c.b, metric, threshold, threshold_common,
                                  greedy ? kSearchNoDiagonal : kSearchUpperOnly);
    ck.qoff = d_rel + c.rel_at;
    ck.c = d_c;
    return ck;
  };
  auto fetch = [&] {
    HIP_CHECK(hipMemcpyAsync(host_out.data(), d_out, out_words * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    std::copy_n(host_out.begin(), n, cluster_out);
    std::copy_n(host_out.begin() + n, n, representative);
    if (rep_common) std::copy_n(host_out.begin() + 2 * (size_t)n, n, rep_common);
    *n_clusters = host_out[out_words - 1];
  };

  if (!greedy) {
    uint32_t* d_parent = ws.take<uint32_t>(n);
    uint32_t* d_work = ws.take<uint32_t>((size_t)n * 4 + 2);
    launch_cluster_iota(d_parent, n, s);
    for (const Chunk& c : chunks) {
      dev.count("cluster_chunk");
      const SearchChunk ck = chunk_of(c);
      if (ck.T == 0) continue;
      HIP_CHECK(hipMemsetAsync(ck.c, 0, (size_t)ck.nq * n * 4, s));
      launch_cluster_probe(dir, ck, dev, s);
      launch_cluster_link(ck, d_parent, dev, s);
    }
    launch_cluster_finish_components(d_parent, scores ? d_scores : nullptr, offsets.as<uint64_t>(), n, d_work, d_out, dev, s);
    fetch();
    return;
  }

  // greedy: the rows of the search kernels stay in HBM, chunk by chunk, until their total is known
  struct Held { SearchRow* rows = nullptr; uint32_t* qrows = nullptr; uint32_t R = 0; };
  std::vector<Held> held(chunks.size());
  uint32_t* d_tiles = ws.take<uint32_t>((size_t)max_q * tiles + 1);
  uint32_t* d_start = ws.take<uint32_t>((size_t)n + 1);
  uint64_t total = 0;
  for (size_t k = 0; k < chunks.size(); k++) {
    dev.count("cluster_chunk");
    SearchChunk ck = chunk_of(chunks[k]);
    if (ck.T == 0) continue;
    ck.tile_rows = d_tiles;
    const uint32_t R = search_chunk_rows(dir, ck, dev, s);
    total += R;
    if (total > g_cluster_pair_budget)
      throw Error(kMsg, "cluster: the greedy linkage holds the directed adjacency in device memory; it has reached " + std::to_string(total) +
                        " entries, the pair budget is " + std::to_string(g_cluster_pair_budget) +
                        " (smh_cluster_set_pair_budget; a higher threshold gives fewer)");
    if (R == 0) continue;
    held[k].R = R;
    held[k].rows = ws.take<SearchRow>(R);
    held[k].qrows = ws.take<uint32_t>(ck.nq);
    launch_search_many_emit(ck, held[k].rows, held[k].qrows, dev, s);
  }
  ClusterAdj* d_adj = ws.take<ClusterAdj>(std::max<uint64_t>(total, 1));
  uint32_t* d_rank = ws.take<uint32_t>(n);
  uint32_t* d_st = ws.take<uint32_t>((size_t)n * 2);
  unsigned long long* d_und = ws.take<unsigned long long>(1);
  uint32_t* d_work = ws.take<uint32_t>((size_t)n * 2 + 1);
  uint32_t base = 0;
  for (size_t k = 0; k < chunks.size(); k++) {
    const Held& h = held[k];
    launch_cluster_pack(h.rows, h.R, h.qrows, chunks[k].b - chunks[k].a, base, d_adj, d_start + chunks[k].a, s);
    base += h.R;
  }
  launch_cluster_pack(nullptr, 0, nullptr, 1, base, d_adj, d_start + n, s);   // start[n] = the entries

  // rank[v] = v's position in priority order: score descending, ties to the lower node
  order.resize(n); rank.resize(n);
  std::iota(order.begin(), order.end(), 0u);
  auto score_of = [&](uint32_t v) { return scores ? scores[v] : (uint32_t)(qoff[v + 1] - qoff[v]); };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return score_of(x) > score_of(y); });
  for (uint32_t p = 0; p < n; p++) rank[order[p]] = p;
  HIP_CHECK(hipMemcpyAsync(d_rank, rank.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));

  uint32_t* st[2] = {d_st, d_st + n};
  HIP_CHECK(hipMemsetAsync(st[0], 0, (size_t)n * 4, s));   // kClusterUndecided
  int cur = 0;
  const uint32_t period = g_cluster_rounds;
  for (unsigned long long undecided = n; undecided != 0;) {
    HIP_CHECK(hipMemsetAsync(d_und, 0, 8, s));
    const bool timed = dev.profiling();   // the timer's entries count the rounds then; else the event counter does
    for (uint32_t r = 0; r < period; r++) {
      if (timed) dev.prof_begin(s); else dev.count("cluster_round");
      launch_cluster_round(d_start, d_adj, d_rank, st[cur], st[cur ^ 1], n, r + 1 == period ? d_und : nullptr, dev, s);
      if (timed) dev.prof_end("cluster_round", s);
      cur ^= 1;
    }
    HIP_CHECK(hipMemcpyAsync(&undecided, d_und, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  launch_cluster_assign(d_start, d_adj, d_rank, st[cur], metric, offsets.as<uint64_t>(), n, d_work, d_out, dev, s);
  fetch();
}

}  // namespace smh
