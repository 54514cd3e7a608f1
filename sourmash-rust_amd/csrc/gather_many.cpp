// gather_many.cpp -- ResidentIndex::gather_many (the rules are in include/sourmash_amd.h,
// smh_index_gather_many): the checks of every query, the staging of a batch of sketches into one CSR in device memory, the
// chunks cut at query boundaries, and per chunk the probe, the sizing, the fill, the rounds and the read-back.  The kernels
// are in gather_many_kernels.hip; the hash directory is the index's (index.cpp), shared with match.
#include <algorithm>
#include <memory>
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
  for (uint32_t q = 0; q < nq; q++) {
    if (qoff[q + 1] < qoff[q]) throw Error(kMsg, "gather_many: offsets must ascend (query " + std::to_string(q) + ")");
    if (qoff[q + 1] - qoff[q] >= 0xffffffffull) throw_internal("gather_many: a query of 2^32 - 1 or more hashes");
  }
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
      PoolBlock d_qoff(((size_t)Qc + 1) * 4), d_pos(T * 8), d_cnt(pairs * 12 + 4), d_qcnt((size_t)Qc * 4), d_qs((size_t)Qc * sizeof(GatherManyQuery)),
          d_st(sizeof(GatherManyState)), d_rowoff((size_t)Qc * 8);
      GatherManyChunk ck;
      ck.hashes = qh + qoff[a];
      ck.counts = qab ? qab + qoff[a] : nullptr;
      ck.qoff = d_qoff.as<uint32_t>();
      ck.nq = Qc; ck.T = (uint32_t)T; ck.n = n;
      ck.rank = d_pos.as<uint32_t>();
      ck.assigned = ck.rank + T;
      ck.c0 = d_cnt.as<uint32_t>();
      ck.c = ck.c0 + pairs;
      ck.loff = ck.c + pairs;
      ck.rowoff = d_rowoff.as<uint64_t>();
      ck.qs = d_qs.as<GatherManyQuery>();
      ck.st = d_st.as<GatherManyState>();
      rel.resize((size_t)Qc + 1);
      for (uint32_t k = 0; k <= Qc; k++) rel[k] = (uint32_t)(qoff[a + k] - qoff[a]);
      HIP_CHECK(hipMemcpyAsync(d_qoff.ptr, rel.data(), ((size_t)Qc + 1) * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemsetAsync(ck.c0, 0, pairs * 8, s));   // c0 and c
      HIP_CHECK(hipMemsetAsync(ck.assigned, 0xff, T * 4, s));
      HIP_CHECK(hipMemsetAsync(ck.st, 0, sizeof(GatherManyState), s));
      launch_gather_many_probe(dir, ck, threshold, d_qcnt.as<uint32_t>(), dev, s);
      qcnt.resize(Qc);
      GatherManyState h_st;
      HIP_CHECK(hipMemcpyAsync(qcnt.data(), d_qcnt.ptr, (size_t)Qc * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(&h_st, ck.st, sizeof h_st, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      auto idle = [&] { d_qoff.synced = d_pos.synced = d_cnt.synced = d_qcnt.synced = d_qs.synced = d_st.synced = d_rowoff.synced = true; };
      if (h_st.hits >= (1ull << 32)) {
        idle();
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
      if (h_st.hits == 0 || R == 0) { blank(qoff[a] - base0, T); idle(); break; }
      const uint32_t hits = (uint32_t)h_st.hits;
      PoolBlock d_lists((size_t)hits * 4), d_rows(R * sizeof(GatherRow));
      ck.lists = d_lists.as<uint32_t>();
      ck.rows = d_rows.as<GatherRow>();
      h_st.live = Qc; h_st.max_rounds = 0;
      HIP_CHECK(hipMemcpyAsync(d_rowoff.ptr, rowoff.data(), (size_t)Qc * 8, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(d_qs.ptr, qs.data(), (size_t)Qc * sizeof(GatherManyQuery), hipMemcpyHostToDevice, s));
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
      HIP_CHECK(hipMemcpyAsync(crow.data(), d_rows.ptr, R * sizeof(GatherRow), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(qs.data(), d_qs.ptr, (size_t)Qc * sizeof(GatherManyQuery), hipMemcpyDeviceToHost, s));
      if (assigned) HIP_CHECK(hipMemcpyAsync(assigned + (qoff[a] - base0), ck.assigned, T * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      idle();
      d_lists.synced = d_rows.synced = true;
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
  // every query as gather() checks it; the lowest failing query decides, and the message names it
  for (uint32_t q = 0; q < nq; q++) {
    const std::string who = "gather_many: query " + std::to_string(q);
    if (queries[q]->num != 0) throw Error(kMsg, who + " is a num sketch; only scaled sketches (num == 0) can be gathered");
    if (any_num) throw Error(kMsg, who + ": the index holds a num sketch; only scaled sketches (num == 0) can be gathered");
    try {
      check_sketch(*queries[q]);
    } catch (const Error& e) {
      throw Error(e.code, who + ": " + e.message);
    }
  }
  check_directory_size("gather_many");
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  // the batch as one CSR in device memory: a state that lives in HBM is copied there device to device, the host states go up
  // in one upload (straight into place when no query lives in HBM)
  std::vector<uint64_t> qoff((size_t)nq + 1, 0);
  bool any_abund = false, any_dev = false;
  uint64_t host_total = 0;
  for (uint32_t q = 0; q < nq; q++) {
    const KmerMinHash& Q = *queries[q];
    Q.flush_pending();
    const uint64_t lq = Q.dev ? Q.dev->n : Q.mins.size();
    if (!Q.dev && Q.has_abunds && Q.abunds.size() != lq)
      throw_internal("gather_many: the abundance vector of query " + std::to_string(q) + " does not match its hashes (quirks Q5/Q6)");
    if (Q.dev && Q.has_abunds && !Q.dev->has_counts && !Q.dev->has_runs)
      throw_internal("gather_many: the device state of query " + std::to_string(q) + " carries no abundances");
    if (lq >= 0xffffffffull) throw_internal("gather_many: a query of 2^32 - 1 or more hashes");
    qoff[q + 1] = qoff[q] + lq;
    any_abund |= Q.has_abunds;
    any_dev |= Q.dev != nullptr;
    if (!Q.dev) host_total += lq;
  }
  const uint64_t total = qoff[nq];
  const size_t words = any_abund ? 2 : 1;
  PoolBlock csr(total * 8 * words);
  uint64_t* d_h = csr.as<uint64_t>();
  uint64_t* d_a = any_abund ? d_h + total : nullptr;
  std::unique_ptr<PoolBlock> up;
  std::vector<uint64_t> stage;
  if (!any_dev) {
    stage.resize(total * words);
    for (uint32_t q = 0; q < nq; q++) {
      const KmerMinHash& Q = *queries[q];
      std::copy(Q.mins.begin(), Q.mins.end(), stage.begin() + qoff[q]);
      if (!any_abund) continue;
      if (Q.has_abunds) std::copy(Q.abunds.begin(), Q.abunds.end(), stage.begin() + total + qoff[q]);
      else std::fill(stage.begin() + total + qoff[q], stage.begin() + total + qoff[q + 1], 1ull);
    }
    if (total) HIP_CHECK(hipMemcpyAsync(d_h, stage.data(), total * 8 * words, hipMemcpyHostToDevice, s));
  } else {
    // host states: [hashes, abundances] of each, one after another
    stage.reserve(host_total * words);
    for (uint32_t q = 0; q < nq; q++) {
      const KmerMinHash& Q = *queries[q];
      if (Q.dev) continue;
      stage.insert(stage.end(), Q.mins.begin(), Q.mins.end());
      if (!any_abund) continue;
      if (Q.has_abunds) stage.insert(stage.end(), Q.abunds.begin(), Q.abunds.end());
      else stage.insert(stage.end(), Q.mins.size(), 1ull);
    }
    up = std::make_unique<PoolBlock>(stage.size() * 8);
    if (!stage.empty()) HIP_CHECK(hipMemcpyAsync(up->ptr, stage.data(), stage.size() * 8, hipMemcpyHostToDevice, s));
    uint64_t at = 0;
    for (uint32_t q = 0; q < nq; q++) {
      const KmerMinHash& Q = *queries[q];
      const uint64_t lq = qoff[q + 1] - qoff[q];
      if (lq == 0) continue;
      if (!Q.dev) {
        HIP_CHECK(hipMemcpyAsync(d_h + qoff[q], up->as<uint64_t>() + at, lq * 8, hipMemcpyDeviceToDevice, s));
        if (any_abund) HIP_CHECK(hipMemcpyAsync(d_a + qoff[q], up->as<uint64_t>() + at + lq, lq * 8, hipMemcpyDeviceToDevice, s));
        at += lq * words;
        continue;
      }
      const DeviceSketch& S = *Q.dev;
      HIP_CHECK(hipMemcpyAsync(d_h + qoff[q], S.uniq.ptr, lq * 8, hipMemcpyDeviceToDevice, s));
      if (!any_abund) continue;
      if (Q.has_abunds && S.has_counts) HIP_CHECK(hipMemcpyAsync(d_a + qoff[q], S.counts.ptr, lq * 8, hipMemcpyDeviceToDevice, s));
      else launch_gather_many_weights(Q.has_abunds ? S.starts.as<uint32_t>() : nullptr, (uint32_t)S.total, (uint32_t)lq, d_a + qoff[q], s);
    }
  }
  HIP_CHECK(hipStreamSynchronize(s));   // (`stage` is read by the upload)
  csr.synced = true;
  if (up) up->synced = true;
  gather_many_dev(d_h, d_a, qoff.data(), nq, threshold, capacity, row_offsets, rows, assigned, dev, s);
  if (query_offsets) std::copy(qoff.begin(), qoff.end(), query_offsets);
}

}  // namespace smh
