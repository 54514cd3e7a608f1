// lca.cpp -- taxonomic LCA on a resident index (the rules are in include/sourmash_amd.h, "Taxonomic LCA"):
// the taxonomy's checks and its copy, the upload and the per-hash table kept beside the hash directory, the sketch route
// (query_batch.cpp's staging, chunks cut at query boundaries, per chunk the probe, the compaction, the sort and the run-length pass) and the
// records route (match's front half, then the fold of the join per record).  The kernels are in lca_kernels.hip.
#include <algorithm>
#include <memory>
#include <string>

#include "index.hpp"

namespace smh {

uint64_t g_lca_budget = kLcaBudget;

namespace {
[[noreturn]] void refuse(const std::string& what) { throw Error(kMsg, "lca: " + what); }
}  // namespace

struct LcaDev {
  DeviceBuffer tax, node_taxon, hash_taxon;
};

void lca_check_taxonomy(const uint32_t* parent, uint32_t n_taxa, const uint32_t* node_taxon, uint32_t n_nodes, uint32_t index_len) {
  if (n_taxa == 0) refuse("n_taxa is 0; a taxonomy holds its root at least");
  if (n_taxa == kLcaNoTaxon) refuse("n_taxa is " + std::to_string(n_taxa) + "; a taxonomy holds fewer than 2^32 - 1 taxa");
  if (n_nodes != index_len)
    refuse("n_nodes is " + std::to_string(n_nodes) + " but the index holds " + std::to_string(index_len) + " nodes");
  if (parent[0] != 0) refuse("parent[0] is " + std::to_string(parent[0]) + "; taxon 0 is the root and its own parent");
  for (uint32_t t = 1; t < n_taxa; t++)
    if (parent[t] >= t)
      refuse("parent[" + std::to_string(t) + "] is " + std::to_string(parent[t]) + "; a parent comes before its children (parent[t] < t)");
  for (uint32_t i = 0; i < n_nodes; i++)
    if (node_taxon[i] != kLcaNoTaxon && node_taxon[i] >= n_taxa)
      refuse("node_taxon[" + std::to_string(i) + "] is " + std::to_string(node_taxon[i]) + "; the taxonomy holds " + std::to_string(n_taxa) +
             " taxa");
}

void ResidentIndex::set_taxonomy(const uint32_t* parent, uint32_t n_taxa, const uint32_t* nt, uint32_t n_nodes) {
  lca_check_taxonomy(parent, n_taxa, nt, n_nodes, n);
  std::vector<uint32_t> p(parent, parent + n_taxa), d(n_taxa, 0), t(nt, nt + n_nodes);
  for (uint32_t k = 1; k < n_taxa; k++) d[k] = d[p[k]] + 1;   // (topological order: one pass)
  if (lca_dev) {
    std::lock_guard<std::recursive_mutex> lock(Device::get().mutex());   // (device state exists: so does the device)
    drop_lca_dev();
  }
  tax_parent.swap(p); tax_depth.swap(d); node_taxon.swap(t);
}

void ResidentIndex::drop_lca_dev() { delete lca_dev; lca_dev = nullptr; }

ResidentIndex::LcaView ResidentIndex::ensure_lca(const MatchDirectory& dir, Device& dev, hipStream_t s) {
  if (!lca_dev) {
    auto L = std::make_unique<LcaDev>();
    const size_t nt = tax_parent.size();
    std::vector<uint64_t> packed(nt);
    for (size_t t = 0; t < nt; t++) packed[t] = ((uint64_t)tax_depth[t] << 32) | tax_parent[t];
    L->tax.ensure(nt * 8);
    L->node_taxon.ensure((size_t)n * 4 + 4);
    L->hash_taxon.ensure((size_t)dir.n_hashes * 4 + 4);
    HIP_CHECK(hipMemcpyAsync(L->tax.ptr, packed.data(), nt * 8, hipMemcpyHostToDevice, s));
    if (n) HIP_CHECK(hipMemcpyAsync(L->node_taxon.ptr, node_taxon.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    const LcaTaxonomy T{L->tax.as<uint64_t>(), L->node_taxon.as<uint32_t>()};
    const size_t longs = (size_t)dir.n_pairs / (kLcaOwnerLaneMax + 1) + 1;
    Workspace ws(s);
    uint32_t* d_long = ws.take<uint32_t>(longs + 1);
    launch_lca_table(dir, T, L->hash_taxon.as<uint32_t>(), d_long, d_long + longs, dev, s);
    HIP_CHECK(hipStreamSynchronize(s));   // (`packed` is read by the upload)
    dev.count("lca_table_built");
    lca_dev = L.release();
  }
  return {{lca_dev->tax.as<uint64_t>(), lca_dev->node_taxon.as<uint32_t>()}, lca_dev->hash_taxon.as<uint32_t>()};
}

void ResidentIndex::check_lca_sketches(const char* who) const {
  if (!has_taxonomy()) throw Error(kMsg, std::string(who) + ": the index has no taxonomy (smh_index_set_taxonomy)");
  if (!(uniform && all_scaled))
    throw Error(kMsg, std::string(who) + ": the index's nodes must be scaled sketches with the same ksize, molecule, seed and max_hash");
}

void ResidentIndex::lca_many_dev(const uint64_t* qh, const uint64_t* qoff, uint32_t nq, uint64_t* count_offsets, std::vector<uint32_t>* taxa_out,
                                 std::vector<uint64_t>* counts_out, uint32_t* hash_taxon, Device& dev, hipStream_t s) {
  check_lca_sketches("lca_many");
  check_query_offsets("lca_many", qoff, nq, kQueryLimit31);
  check_directory_size("lca_many");
  const uint64_t total = nq ? qoff[nq] - qoff[0] : 0, base0 = nq ? qoff[0] : 0;
  std::vector<uint64_t> coff((size_t)nq + 1, 0);
  std::vector<uint32_t> taxa;
  std::vector<uint64_t> counts;
  auto finish = [&] {
    std::copy(coff.begin(), coff.end(), count_offsets);
    taxa_out->swap(taxa);
    counts_out->swap(counts);
  };
  auto blank = [&](uint64_t from, uint64_t len) { if (hash_taxon) std::fill(hash_taxon + from, hash_taxon + from + len, kLcaNoTaxon); };
  if (n == 0 || total == 0) { blank(0, total); finish(); return; }

  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  const MatchDirectory dir = ensure_directory("lca_many", dev, s);
  if (dir.n_hashes == 0) { blank(0, total); finish(); return; }
  const LcaView L = ensure_lca(dir, dev, s);
  const uint64_t budget = std::max<uint64_t>(g_lca_budget, 1);
  std::vector<uint32_t> rel;
  std::vector<uint64_t> h_keys, h_cnt, per;

  for (uint32_t a = 0, b = 0; a < nq; a = b) {
    // the chunk: queries while their hashes fit the budget (and 2^31 - 1 positions, what the sort takes); one at least
    b = a + 1;
    while (b < nq && qoff[b + 1] - qoff[a] <= budget && qoff[b + 1] - qoff[a] < (1ull << 31)) b++;
    const uint32_t Qc = b - a;
    const uint32_t T = (uint32_t)(qoff[b] - qoff[a]);
    dev.count("lca_chunk");
    for (uint32_t q = a; q < b; q++) coff[q + 1] = coff[q];
    if (T == 0) continue;
    Workspace ws(s);
    uint32_t* d_qoff = ws.take<uint32_t>((size_t)Qc + 1);
    uint32_t* d_tax = ws.take<uint32_t>(T);
    uint64_t* d_key = ws.take<uint64_t>(T);
    uint32_t* d_flag = ws.take<uint32_t>((size_t)T + 1);
    upload_chunk_offsets(qoff, a, b, &rel, d_qoff, s);
    launch_lca_probe(dir, L.hash_taxon, qh + qoff[a], d_qoff, Qc, T, d_tax, d_key, d_flag, dev, s);
    if (hash_taxon) HIP_CHECK(hipMemcpyAsync(hash_taxon + (qoff[a] - base0), d_tax, (size_t)T * 4, hipMemcpyDeviceToHost, s));
    uint32_t* total_dev = d_flag + T;
    uint32_t nkeys = 0;
    exclusive_scan_u32_dev(d_flag, T, total_dev, dev.scratch, s);
    HIP_CHECK(hipMemcpyAsync(&nkeys, total_dev, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));   // (`rel` is read by the upload)
    if (nkeys == 0) continue;
    // the assigned keys compacted, sorted, run-length encoded: the runs are (query, taxon) ascending with their counts
    uint64_t* k[2] = {ws.take<uint64_t>(nkeys), ws.take<uint64_t>(nkeys)};
    uint64_t* d_uniq = ws.take<uint64_t>(nkeys);
    uint32_t* d_starts = ws.take<uint32_t>((size_t)nkeys + 1);
    launch_lca_keys(d_key, d_flag, T, k[0], dev, s);
    const int cur = radix_sort_u64_keys(k[0], k[1], nkeys, dev.scratch, s, 0);
    const uint32_t nruns = run_length_encode_u64(k[cur], nkeys, d_uniq, d_starts, dev.scratch, s);
    uint64_t* d_cnt = k[cur ^ 1];   // (the sort's other half is free now: nruns <= nkeys)
    starts_to_counts(d_starts, nruns, nkeys, d_cnt, s);
    h_keys.resize(nruns); h_cnt.resize(nruns);
    HIP_CHECK(hipMemcpyAsync(h_keys.data(), d_uniq, (size_t)nruns * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(h_cnt.data(), d_cnt, (size_t)nruns * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    per.assign(Qc, 0);
    for (uint32_t r = 0; r < nruns; r++) {
      taxa.push_back((uint32_t)h_keys[r]);
      counts.push_back(h_cnt[r]);
      per[(uint32_t)(h_keys[r] >> 32)]++;
    }
    for (uint32_t k = 0; k < Qc; k++) coff[(size_t)a + k + 1] = coff[(size_t)a + k] + per[k];
  }
  finish();
}

void ResidentIndex::lca_many(const KmerMinHash* const* queries, uint32_t nq, uint64_t* count_offsets, std::vector<uint32_t>* taxa,
                             std::vector<uint64_t>* counts, uint64_t* query_offsets, uint32_t* hash_taxon, Device& dev) {
  check_lca_sketches("lca_many");
  check_queries("lca_many", "have lca counts", queries, nq);   // (the index holds no num sketch: check_lca_sketches)
  check_directory_size("lca_many");
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  const QueryBatch batch(queries, nq, "lca_many", kQueryLimit31, false, dev);
  lca_many_dev(batch.hashes(), batch.offsets(), nq, count_offsets, taxa, counts, hash_taxon, dev, dev.stream());
  if (query_offsets) std::copy_n(batch.offsets(), (size_t)nq + 1, query_offsets);
}

void ResidentIndex::lca_records(const uint8_t* seq_dev, uint64_t total_len, const uint64_t* off, uint32_t nrec, LcaRow* rows, hipStream_t s) {
  check_match_batch(off, nrec, total_len);
  if (!has_taxonomy()) throw Error(kMsg, "lca_records: the index has no taxonomy (smh_index_set_taxonomy)");
  auto blank = [&](uint32_t a, uint32_t e) { for (uint32_t r = a; r < e; r++) rows[r] = LcaRow{0, 0, 0, 0, kLcaNoTaxon, 0}; };
  auto tail = [&](const MatchDirectory& dir, const MatchFold& f) {
    Device& dev = Device::get();
    const LcaView L = ensure_lca(dir, dev, s);
    Workspace ws(s);
    LcaRow* d_out = ws.take<LcaRow>(f.nf);
    uint32_t* d_big = ws.take<uint32_t>((size_t)f.nf + 1);
    launch_lca_records(L.tax, L.hash_taxon, f.rank, f.rows, f.rec_first, f.nf, d_out, d_big, d_big + f.nf, dev, s);
    fetch_rows(d_out, rows + f.f0, f.nf, Engine::get(), s);
  };
  match_folds(seq_dev, total_len, off, nrec, false, s, blank, tail);
}

}  // namespace smh
