// gather_many.cpp -- ResidentIndex::gather_many (the rules are in include/sourmash_amd.h,
// smh_index_gather_many): the chunks cut at query boundaries, and per chunk the probe, the sizing, the fill, the rounds and
// the read-back.  The checks of every query and the staging of a batch of sketches into one CSR in device memory are
// query_batch.cpp's.  The kernels are in gather_many_kernels.hip; the hash directory is the index's (index.cpp), shared with
// match.
#include <algorithm>
#include <string>

#include "index.hpp"

namespace smh {

uint64_t g_gather_many_budget = kGatherManyBudget;

uint32_t query_chunk_end(const uint64_t* qoff, uint32_t a, uint32_t nq, uint32_t n_nodes, uint64_t budget, uint32_t max_queries) {
  const uint64_t per = std::min<uint64_t>(std::max<uint64_t>(budget / std::max(n_nodes, 1u), 1), max_queries);
  uint32_t b = (uint32_t)std::min<uint64_t>(nq, a + per);
  while (b > a + 1 && qoff[b] - qoff[a] >= 0xffffffffull) b--;
  return b;
}

uint32_t gather_many_chunk_end(const uint64_t* qoff, uint32_t a, uint32_t nq, uint32_t n_nodes, uint64_t budget) {
  return query_chunk_end(qoff, a, nq, n_nodes, budget, kGatherManyMaxQueries);
}

void ResidentIndex::gather_many_dev(const uint64_t* qh, const uint64_t* qab, const uint64_t* qoff, uint32_t nq, uint32_t threshold,
                                    uint32_t capacity, uint64_t* row_offsets, std::vector<GatherRow>* rows_out, uint32_t* assigned,
                                    Device& dev, hipStream_t s) {
  if (threshold == 0) threshold = 1;
  check_query_offsets("gather_many", qoff, nq, kQueryLimit32);
  check_directory_size("gather_many");
  const uint64_t total = nq ? qoff[nq] - qoff[0] : 0;
  std::vector<uint64_t> roff((size_t)nq + 1, 0);
  std::vector<GatherRow> out;
  // `assigned` is written in place, chunk by chunk (the refusals above come first: they write nothing)
  auto blank = [&](uint64_t from, uint64_t len) { if (assigned) std::fill(assigned + from, assigned + from + len, 0xffffffffu); };
  auto finish = [&] {
    std::copy(roff.begin(), roff.end(), row_offsets);
    rows_out->swap(out);
  };
  if (n == 0 || total == 0) { blank(0, total); finish(); return; }

  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  const MatchDirectory dir = ensure_directory("gather_many", dev, s);
  if (dir.n_hashes == 0) { blank(0, total); finish(); return; }
  const uint64_t base0 = qoff[0];
  std::vector<uint32_t> rel, qcnt;
  std::vector<uint64_t> rowoff;
  std::vector<GatherManyQuery> qs;
  std::vector<GatherRow> crow;

  for (uint32_t a = 0, b = 0; a < nq; a = b) {
    b = gather_many_chunk_end(qoff, a, nq, n, g_gather_many_budget);
    for (;;) {   // (again with half the queries when the chunk's hits do not fit 32 bits)
      const uint32_t Qc = b - a;
      const uint64_t T = qoff[b] - qoff[a];
      for (uint32_t q = a; q < b; q++) roff[q + 1] = roff[q];
      if (T == 0) { dev.count("gather_many_chunk"); break; }
      const size_t pairs = (size_t)Qc * n;
      Workspace ws(s);
      GatherManyChunk ck;
      ck.hashes = qh + qoff[a];
      ck.counts = qab ? qab + qoff[a] : nullptr;
      uint32_t* d_qoff = ws.take<uint32_t>((size_t)Qc + 1);
      ck.qoff = d_qoff;
      ck.nq = Qc; ck.T = (uint32_t)T; ck.n = n;
      ck.rank = ws.take<uint32_t>(T * 2);
      ck.assigned = ck.rank + T;
      ck.c0 = ws.take<uint32_t>(pairs * 3 + 1);
      ck.c = ck.c0 + pairs;
      ck.loff = ck.c + pairs;
      uint32_t* d_qcnt = ws.take<uint32_t>(Qc);
      ck.qs = ws.take<GatherManyQuery>(Qc);
      ck.st = ws.take<GatherManyState>(1);
      uint64_t* d_rowoff = ws.take<uint64_t>(Qc);
      ck.rowoff = d_rowoff;
      upload_chunk_offsets(qoff, a, b, &rel, d_qoff, s);   // (the stream is waited for below, on every way on)
      HIP_CHECK(hipMemsetAsync(ck.c0, 0, pairs * 8, s));   // c0 and c
      HIP_CHECK(hipMemsetAsync(ck.assigned, 0xff, T * 4, s));
      HIP_CHECK(hipMemsetAsync(ck.st, 0, sizeof(GatherManyState), s));
      launch_gather_many_probe(dir, ck, threshold, d_qcnt, dev, s);
      qcnt.resize(Qc);
      GatherManyState h_st;
      HIP_CHECK(hipMemcpyAsync(qcnt.data(), d_qcnt, (size_t)Qc * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(&h_st, ck.st, sizeof h_st, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (h_st.hits >= (1ull << 32)) {
        if (Qc == 1) throw_internal("gather_many: 2^32 or more (sketch, query hash) matches of one query");
        b = a + Qc / 2;
        continue;
      }
      dev.count("gather_many_chunk");
      // a query writes at most min(capacity, nodes that reach the threshold) rows
      rowoff.resize(Qc);
      qs.assign(Qc, GatherManyQuery{0, 0, 0, 0});
      uint64_t R = 0;
      uint32_t max_cap = 0, max_lq = 0;
      for (uint32_t k = 0; k < Qc; k++) {
        rowoff[k] = R;
        qs[k].cap = std::min(capacity, qcnt[k]);
        R += qs[k].cap;
        max_cap = std::max(max_cap, qs[k].cap);
        max_lq = std::max(max_lq, rel[k + 1] - rel[k]);
      }
      if (h_st.hits == 0 || R == 0) { blank(qoff[a] - base0, T); break; }
      const uint32_t hits = (uint32_t)h_st.hits;
      ck.lists = ws.take<uint32_t>(hits);
      ck.rows = ws.take<GatherRow>(R);
      h_st.live = Qc; h_st.max_rounds = 0;
      HIP_CHECK(hipMemcpyAsync(d_rowoff, rowoff.data(), (size_t)Qc * 8, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(ck.qs, qs.data(), (size_t)Qc * sizeof(GatherManyQuery), hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(ck.st, &h_st, 8, hipMemcpyHostToDevice, s));
      launch_gather_many_fill(dir, ck, dev, s);
      // every query is done after its cap + 1 picks at the latest
      const uint32_t sub_grid = grid_for(std::min(max_len, max_lq), 1024, 32, dev);
      for (uint64_t queued = 0;;) {
        launch_gather_many_rounds(dir, ck, offsets.as<uint64_t>(), threshold, sub_grid, kGatherRoundsPerSync, dev, s);
        queued += kGatherRoundsPerSync;
        HIP_CHECK(hipMemcpyAsync(&h_st, ck.st, 8, hipMemcpyDeviceToHost, s));   // {live, max_rounds}
        HIP_CHECK(hipStreamSynchronize(s));
        if (h_st.live == 0) break;
        if (queued > max_cap) throw_internal("gather_many: queries still live after every round they can take");
      }
      crow.resize(R);
      HIP_CHECK(hipMemcpyAsync(crow.data(), ck.rows, R * sizeof(GatherRow), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(qs.data(), ck.qs, (size_t)Qc * sizeof(GatherManyQuery), hipMemcpyDeviceToHost, s));
      if (assigned) HIP_CHECK(hipMemcpyAsync(assigned + (qoff[a] - base0), ck.assigned, T * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      for (uint32_t k = 0; k < Qc; k++) {
        out.insert(out.end(), crow.begin() + rowoff[k], crow.begin() + rowoff[k] + qs[k].rounds);
        roff[a + k + 1] = roff[a + k] + qs[k].rounds;
      }
      break;
    }
  }
  finish();
}

void ResidentIndex::gather_many(const KmerMinHash* const* queries, uint32_t nq, uint32_t threshold, uint32_t capacity, uint64_t* row_offsets,
                                std::vector<GatherRow>* rows, uint64_t* query_offsets, uint32_t* assigned, Device& dev) {
  check_queries("gather_many", "can be gathered", queries, nq);
  check_directory_size("gather_many");
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  const QueryBatch batch(queries, nq, "gather_many", kQueryLimit32, true, dev);
  gather_many_dev(batch.hashes(), batch.abunds(), batch.offsets(), nq, threshold, capacity, row_offsets, rows, assigned, dev, dev.stream());
  if (query_offsets) std::copy_n(batch.offsets(), (size_t)nq + 1, query_offsets);
}

}  // namespace smh
