// match.cpp -- ResidentIndex::match (the rules are in include/sourmash_amd.h, "Matching records"): the folds
// of a batch cut at record boundaries (the index's hash directory is index.cpp's), and per fold the grouped fold's own
// sequence (hash with positions, positions to records, two sorts, the two-key run-length pass) followed by the probe, the
// tally with its two regimes and the read-back.  The kernels are in match_kernels.hip.  Everything up to the probe is
// match_folds, which lca.cpp's records route runs too; what follows the probe is the caller's `tail`.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>

#include "index.hpp"

namespace smh {

uint64_t g_match_pair_budget = kMatchPairBudget;

namespace {
[[noreturn]] void refuse(const std::string& what) { throw Error(kMsg, "match: " + what); }
}  // namespace

// The rows of a fold into the caller's pageable array through two page-locked halves: the copy out of one half runs while
// the transfer into the other is in flight (a pageable destination would be staged by the runtime, one piece after another).
static_assert(sizeof(MatchRow) == sizeof(LcaRow), "fetch_rows serves both row types");
void fetch_rows(const void* d_rows_v, void* out_v, size_t n, Engine& E, hipStream_t s) {
  const MatchRow* d_rows = static_cast<const MatchRow*>(d_rows_v);
  MatchRow* out = static_cast<MatchRow*>(out_v);
  constexpr size_t kHalf = 1u << 16;   // rows per half: 1.5 MiB
  const size_t half = std::min(n, kHalf);
  E.pin_a.ensure(2 * half * sizeof(MatchRow));
  MatchRow* pin = E.pin_a.as<MatchRow>();
  size_t done = 0, len = half;
  int cur = 0;
  HIP_CHECK(hipMemcpyAsync(pin, d_rows, len * sizeof(MatchRow), hipMemcpyDeviceToHost, s));
  while (done < n) {
    HIP_CHECK(hipStreamSynchronize(s));
    const size_t next = done + len, nlen = std::min(half, n - next);
    if (nlen) HIP_CHECK(hipMemcpyAsync(pin + (size_t)(cur ^ 1) * half, d_rows + next, nlen * sizeof(MatchRow), hipMemcpyDeviceToHost, s));
    memcpy(out + done, pin + (size_t)cur * half, len * sizeof(MatchRow));
    done = next; len = nlen; cur ^= 1;
  }
}

void ResidentIndex::check_matchable() const {
  if (n == 0) refuse("the index holds no node (ksize, seed and max_hash are those of node 0)");
  for (uint32_t i = 0; i < n; i++) {
    const KmerMinHash& p = params[i];
    if (p.molecule != kMoleculeDNA)
      refuse("node " + std::to_string(i) + " is a " + molecule_name(p.molecule) + " sketch; only DNA sketches can be matched");
    if (!(p.num == 0 && p.max_hash != 0))
      refuse("node " + std::to_string(i) + " is not a scaled sketch (num = " + std::to_string(p.num) + ", max_hash = " +
             std::to_string(p.max_hash) + ")");
    const KmerMinHash& p0 = params[0];
    if (p.ksize != p0.ksize || p.seed != p0.seed || p.max_hash != p0.max_hash)
      refuse("node " + std::to_string(i) + " (ksize = " + std::to_string(p.ksize) + ", seed = " + std::to_string(p.seed) + ", max_hash = " +
             std::to_string(p.max_hash) + ") differs from node 0 (ksize = " + std::to_string(p0.ksize) + ", seed = " +
             std::to_string(p0.seed) + ", max_hash = " + std::to_string(p0.max_hash) + ")");
  }
}

void ResidentIndex::check_match_batch(const uint64_t* off, uint32_t nrec, uint64_t total_len) const {
  check_matchable();
  for (uint32_t r = 0; r < nrec; r++)
    if (off[r + 1] < off[r]) refuse("offsets must ascend (record " + std::to_string(r) + ")");
  if (nrec && off[nrec] > total_len)
    refuse("the last offset " + std::to_string(off[nrec]) + " lies beyond the batch's " + std::to_string(total_len) + " bytes");
}

void ResidentIndex::match_folds(const uint8_t* seq_dev, uint64_t total_len, const uint64_t* off, uint32_t nrec, bool want_hits,
                                hipStream_t s, const std::function<void(uint32_t, uint32_t)>& blank,
                                const std::function<void(const MatchDirectory&, const MatchFold&)>& tail) {
  const uint32_t ksize = params[0].ksize;
  const uint64_t seed = params[0].seed, max_hash = params[0].max_hash;
  bool any_long = false;
  for (uint32_t r = 0; r < nrec; r++) any_long |= off[r + 1] - off[r] >= ksize;
  if (!any_long || ksize == 0) { blank(0, nrec); return; }

  Device& dev = Device::get();
  Engine& E = Engine::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  const MatchDirectory dir = ensure_directory("match", dev, s);

  E.offbuf.ensure((size_t)(nrec + 1) * 8);
  E.grpbuf.ensure((size_t)nrec * 4);
  std::vector<uint32_t> identity(nrec);
  std::iota(identity.begin(), identity.end(), 0u);
  HIP_CHECK(hipMemcpyAsync(E.offbuf.ptr, off, (size_t)(nrec + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(E.grpbuf.ptr, identity.data(), (size_t)nrec * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));   // (identity is a stack-lifetime staging vector)
  SeqBatch b;
  b.seq = seq_dev; b.len = total_len; b.starts = E.offbuf.as<uint64_t>(); b.nrec = nrec; b.vend0 = total_len;

  // Folds: consecutive records while their cost -- one per record plus the expected candidates of its bytes -- fits the
  // budget; a record alone always makes a fold, up to what one chunk of candidates can hold.
  const double frac = (double)(((long double)max_hash + 1.0L) / 18446744073709551616.0L);
  const double hard = 1.6e9;   // (estimate_capacity adds a quarter and 64 Ki: below 2^31)
  const double budget = std::min((double)std::max<uint64_t>(g_match_pair_budget, 1), hard);
  for (uint32_t r0 = 0; r0 < nrec;) {
    double cost = 0;
    uint32_t r1 = r0;
    while (r1 < nrec) {
      const double c = 1.0 + (double)(off[r1 + 1] - off[r1]) * frac;
      if (c > hard)
        refuse("record " + std::to_string(r1) + " (" + std::to_string(off[r1 + 1] - off[r1]) + " bytes) alone would leave about " +
               std::to_string((uint64_t)c) + " candidates; one fold takes fewer than 2^31 and no record is split");
      if (r1 > r0 && cost + c > budget) break;
      cost += c;
      r1++;
    }
    const uint32_t nf = r1 - r0;
    const uint64_t lo = off[r0], hi = off[r1];
    const uint32_t f0 = r0;
    r0 = r1;
    const uint64_t nc = hi == lo ? 0 : E.run_dna_chunk(b, ksize, seed, lo, hi, max_hash, s);
    if (nc == 0) { blank(f0, r1); continue; }
    dev.count("match_fold");
    // (hash, position) -> (hash, record); sort by hash, then stably by record; one run per distinct (record, hash)
    launch_pos_to_group(E.cand_pos[0].as<uint64_t>(), nc, E.offbuf.as<uint64_t>(), nrec, E.grpbuf.as<uint32_t>(), s, 0);
    const int c1 = radix_sort_u64(E.cand_hash[0].as<uint64_t>(), E.cand_hash[1].as<uint64_t>(), E.cand_pos[0].as<uint64_t>(),
                                  E.cand_pos[1].as<uint64_t>(), nc, dev.scratch, s);
    const int c2 = radix_sort_u64(E.cand_pos[c1].as<uint64_t>(), E.cand_pos[c1 ^ 1].as<uint64_t>(), E.cand_hash[c1].as<uint64_t>(),
                                  E.cand_hash[c1 ^ 1].as<uint64_t>(), nc, dev.scratch, s, 0, 8);
    const int cur = c1 ^ c2;
    E.ensure_runs(nc); E.uniq2.ensure(nc * 8);
    const uint32_t nruns = run_length_encode_u64(E.cand_hash[cur].as<uint64_t>(), nc, E.uniq.as<uint64_t>(), E.starts.as<uint32_t>(),
                                                 dev.scratch, s, nullptr, nullptr, E.cand_pos[cur].as<uint64_t>(), E.uniq2.as<uint64_t>(), 0);
    if (nruns == 0) { blank(f0, r1); continue; }

    Workspace ws(s);
    MatchFold f;
    f.f0 = f0; f.nf = nf; f.nruns = nruns;
    f.run_hash = E.uniq.as<uint64_t>();
    f.rows = ws.take<MatchRow>(nf);
    f.rec_first = ws.take<uint32_t>(nf);
    f.rec_pairs = ws.take<unsigned long long>(nf);
    f.rank = ws.take<uint32_t>(nruns);
    uint32_t* d_flag = ws.take<uint32_t>(want_hits ? (size_t)nruns + 1 : 1);
    f.hit_flag = want_hits ? d_flag : nullptr;
    HIP_CHECK(hipMemsetAsync(f.rows, 0, (size_t)nf * sizeof(MatchRow), s));
    HIP_CHECK(hipMemsetAsync(f.rec_first, 0xff, (size_t)nf * 4, s));
    HIP_CHECK(hipMemsetAsync(f.rec_pairs, 0, (size_t)nf * 8, s));
    launch_match_probe(dir, E.uniq.as<uint64_t>(), E.uniq2.as<uint64_t>(), E.starts.as<uint32_t>(), nruns, (uint32_t)nc, f0, f.rows, f.rec_first,
                       f.rec_pairs, f.rank, f.hit_flag, dev, s);
    tail(dir, f);
    HIP_CHECK(hipStreamSynchronize(s));
  }
}

void ResidentIndex::match(const uint8_t* seq_dev, uint64_t total_len, const uint64_t* off, uint32_t nrec, MatchRow* rows, uint64_t* hit_offsets,
                          std::vector<uint64_t>* hit_hashes, hipStream_t s) {
  // the rows of records no fold's kernels see (a batch without a window, a fold without a candidate); the others come
  // back whole from the device
  auto blank = [&](uint32_t a, uint32_t e) { for (uint32_t r = a; r < e; r++) rows[r] = MatchRow{0, 0, 0, 0, kMatchMiss, 0}; };
  check_match_batch(off, nrec, total_len);   // (in front of the first write)
  if (hit_offsets) std::fill(hit_offsets, hit_offsets + nrec + 1, 0);
  if (hit_hashes) hit_hashes->clear();
  const bool want_hits = hit_offsets != nullptr;
  auto tail = [&](const MatchDirectory& dir, const MatchFold& f) {
    Device& dev = Device::get();
    Engine& E = Engine::get();
    const uint32_t nf = f.nf;
    Workspace ws(s);
    uint32_t* d_big = ws.take<uint32_t>((size_t)nf + 1);
    uint32_t* big_count = d_big + nf;
    HIP_CHECK(hipMemsetAsync(big_count, 0, 4, s));
    launch_match_tally(dir, f.rank, f.rows, f.rec_first, f.rec_pairs, nf, d_big, big_count, dev, s);
    uint32_t nbig = 0;
    HIP_CHECK(hipMemcpyAsync(&nbig, big_count, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (nbig) {
      // the dense regime, in rounds of as many records as the budget holds counters for (n per record; one at least)
      std::vector<uint32_t> big(nbig);
      HIP_CHECK(hipMemcpyAsync(big.data(), d_big, (size_t)nbig * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      std::sort(big.begin(), big.end());   // (the kernel appended them in any order)
      HIP_CHECK(hipMemcpyAsync(d_big, big.data(), (size_t)nbig * 4, hipMemcpyHostToDevice, s));
      const uint32_t per = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(g_match_pair_budget / n, 1), std::min<uint32_t>(nbig, 1u << 16));
      Workspace dense(s);
      uint32_t* slab = dense.take<uint32_t>((size_t)per * n);
      for (uint32_t at = 0; at < nbig; at += per) {
        launch_match_dense(dir, f.rank, f.rows, f.rec_first, d_big + at, std::min(per, nbig - at), n, slab, dev, s);
        dev.count("match_dense_round");
      }
      HIP_CHECK(hipStreamSynchronize(s));   // (big is read by the upload above)
    }
    fetch_rows(f.rows, rows + f.f0, nf, E, s);
    if (want_hits) {
      uint32_t* total_dev = f.hit_flag + f.nruns;
      uint32_t nhit = 0;
      exclusive_scan_u32_dev(f.hit_flag, f.nruns, total_dev, dev.scratch, s);
      HIP_CHECK(hipMemcpyAsync(&nhit, total_dev, 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (nhit) {
        Workspace hits(s);
        uint64_t* d_hits = hits.take<uint64_t>(nhit);
        launch_match_hit_scatter(f.run_hash, f.rank, f.hit_flag, f.nruns, d_hits, dev, s);
        const size_t have = hit_hashes->size();
        hit_hashes->resize(have + nhit);
        HIP_CHECK(hipMemcpyAsync(hit_hashes->data() + have, d_hits, (size_t)nhit * 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
      }
    }
  };
  match_folds(seq_dev, total_len, off, nrec, want_hits, s, blank, tail);
  // folds follow the records and a fold's hit runs follow (record, hash): the list is the CSR already
  if (hit_offsets)
    for (uint32_t r = 0; r < nrec; r++) hit_offsets[r + 1] = hit_offsets[r] + rows[r].hit_distinct;
}

}  // namespace smh

