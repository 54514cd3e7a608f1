// index_build.cpp -- a ResidentIndex built from records on the device, and the concatenation of resident indexes (DESIGN.md
// 3.19; the rules are in include/sourmash_amd.h, "Building an index from records").  The front half is the grouped fold's own:
// the batch's position space behind a BatchSource, cut into folds of about `budget` expected candidates, each hashed by
// Engine::run_chunk, mapped to groups and sorted by hash, then stably by group.  Where fold_groups (minhash.cpp) goes to the
// host, the kernels of index_build_kernels.hip go on: heads per tile, their scan, the ordered emit and the runs' counts.  The
// runs of several folds are merged by one more sort and the same kernels with the counts as weights.  Per fold the candidate
// count and the run count come to the host, per call the offsets; no hash does.
#include <algorithm>
#include <string>
#include <vector>

#include "index.hpp"

namespace smh {

uint64_t g_index_build_budget = kIndexBuildBudget;

namespace {

[[noreturn]] void refuse(const std::string& what) { throw Error(kMsg, "index build: " + what); }
[[noreturn]] void refuse_concat(const std::string& what) { throw Error(kMsg, "index concat: " + what); }

constexpr uint64_t kMaxPairs = (1ull << 31) - 1;   // what the directory and the compare kernels take

// the runs of one fold, or of all of them merged: ascending by (group, hash)
struct Runs {
  Workspace ws;   // the two blocks: they move with the runs and go back where the runs die
  uint64_t* hash = nullptr;
  uint64_t* pack = nullptr;   // n u64 each; pack: (group << kBuildCountBits) | count
  uint64_t n = 0;
  explicit Runs(hipStream_t s) : ws(s) {}
};

// n elements sorted by (tag >> shift, hash) -> their runs.  The stream is idle when it returns.
Runs runs_of(const uint64_t* hash, const uint64_t* tag, uint64_t n, int shift, uint32_t* err, Device& dev, hipStream_t s) {
  Runs out(s);
  const uint32_t tiles = index_build_tiles(n);
  Workspace ws(s);
  uint32_t* d_tiles = ws.take<uint32_t>((size_t)tiles + 1);
  launch_index_build_heads(hash, tag, n, shift, d_tiles, dev, s);
  exclusive_scan_u32_dev(d_tiles, tiles, d_tiles + tiles, dev.scratch, s);
  uint32_t nruns = 0;
  HIP_CHECK(hipMemcpyAsync(&nruns, d_tiles + tiles, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  out.n = nruns;
  out.hash = out.ws.take<uint64_t>(nruns);
  out.pack = out.ws.take<uint64_t>(nruns);
  uint32_t* d_start = ws.take<uint32_t>(nruns);
  launch_index_build_emit(hash, tag, n, shift, d_tiles, out.hash, d_start, dev, s);
  launch_index_build_counts(tag, n, shift, d_start, nruns, out.pack, err, dev, s);
  HIP_CHECK(hipStreamSynchronize(s));
  return out;
}

// the runs of several folds -> one: a hash of one group that shows up in several folds is one hash with the counts added
Runs merge_runs(std::vector<Runs>& folds, uint32_t* err, Device& dev, hipStream_t s) {
  uint64_t N = 0;
  for (const Runs& r : folds) N += r.n;
  Workspace ws(s);
  uint64_t* k[2] = {ws.take<uint64_t>(N), ws.take<uint64_t>(N)};
  uint64_t* v[2] = {ws.take<uint64_t>(N), ws.take<uint64_t>(N)};
  uint64_t at = 0;
  for (const Runs& r : folds) {
    if (r.n == 0) continue;
    HIP_CHECK(hipMemcpyAsync(k[0] + at, r.hash, r.n * 8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(v[0] + at, r.pack, r.n * 8, hipMemcpyDeviceToDevice, s));
    at += r.n;
  }
  HIP_CHECK(hipStreamSynchronize(s));
  folds.clear();
  // by hash, then stably by the group's bytes above the count: (group, hash) order
  dev.prof_begin(s);
  const int c1 = radix_sort_u64(k[0], k[1], v[0], v[1], N, dev.scratch, s);
  const int c2 = radix_sort_u64(v[c1], v[c1 ^ 1], k[c1], k[c1 ^ 1], N, dev.scratch, s, kBuildCountBits / 8, 8);
  dev.prof_end("index_build_merge", s);
  const int cur = c1 ^ c2;
  return runs_of(k[cur], v[cur], N, kBuildCountBits, err, dev, s);
}

}  // namespace

void check_index_build(const KmerMinHash* like, int input, bool have_seq, uint64_t total_len, const uint64_t* off, const uint32_t* groups,
                       uint32_t nrec, uint32_t G) {
  if (!like) refuse("like is NULL");
  if (!off) refuse("offsets is NULL");
  if (!have_seq && total_len) refuse("seq is NULL");
  if (input != kBuildNucleotide && input != kBuildAmino) refuse("unknown input " + std::to_string(input));
  if (!(like->num == 0 && like->max_hash != 0))
    refuse("`like` is not a scaled sketch (num = " + std::to_string(like->num) + ", max_hash = " + std::to_string(like->max_hash) +
           "); bottom-num nodes are not built on the device");
  if (input == kBuildAmino && like->molecule == kMoleculeDNA) refuse("amino-acid input needs a protein, dayhoff or hp sketch");
  for (uint32_t r = 0; r < nrec; r++)
    if (off[r + 1] < off[r]) refuse("offsets must ascend (record " + std::to_string(r) + ")");
  if (nrec && off[nrec] > total_len)
    refuse("the last offset " + std::to_string(off[nrec]) + " lies beyond the batch's " + std::to_string(total_len) + " bytes");
  if (groups) {
    for (uint32_t r = 0; r < nrec; r++)
      if (groups[r] >= G)
        refuse("groups[" + std::to_string(r) + "] is " + std::to_string(groups[r]) + "; there are " + std::to_string(G) + " groups");
  } else if (G != nrec) {
    refuse("groups is NULL (record r is node r) but n_groups is " + std::to_string(G) + " and there are " + std::to_string(nrec) + " records");
  }
  // slice::windows(0) of the grouped path (a panic there; a refusal here, before anything is built)
  if (like->molecule == kMoleculeDNA ? like->ksize == 0 : like->ksize / 3 == 0) refuse("window size must be non-zero");
  if (G >= (1u << 24))
    refuse("n_groups is " + std::to_string(G) + "; the grouped fold tags a candidate with its group in 24 bits, so a call builds fewer "
           "than 2^24 nodes (concat joins the pieces)");
}

ResidentIndex::ResidentIndex(const KmerMinHash& like, int input, const uint8_t* seq_dev, uint64_t total_len, const uint64_t* off,
                             const uint32_t* groups, uint32_t nrec, uint32_t G, hipStream_t s) {
  check_index_build(&like, input, seq_dev != nullptr, total_len, off, groups, nrec, G);
  n = G;
  h_nums.assign(n, 0);
  params.assign(n, KmerMinHash(0, like.ksize, (Molecule)like.molecule, like.seed, like.max_hash, false));
  has_abunds = like.has_abunds;
  h_offsets.assign((size_t)n + 1, 0);
  const BatchSource::Kind kind = input == kBuildAmino ? BatchSource::kAmino
                                 : like.molecule == kMoleculeDNA ? BatchSource::kDna : BatchSource::kTranslated;
  const uint32_t window = kind == BatchSource::kAmino ? like.ksize / 3 : like.ksize;
  bool any_long = false;
  for (uint32_t r = 0; r < nrec; r++) any_long |= off[r + 1] - off[r] >= window;

  auto& dev = Device::get();
  Engine& E = Engine::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  Runs result(s);
  if (any_long && G) {
    // the sources are exercised on batches of two records and more: a single record gets an empty one behind it
    std::vector<uint64_t> off1;
    std::vector<uint32_t> grp1;
    if (nrec == 1) {
      off1 = {off[0], off[1], off[1]};
      off = off1.data();
      if (groups) { grp1 = {groups[0], groups[0]}; groups = grp1.data(); }
      nrec = 2;
    }
    const uint32_t per = kind == BatchSource::kTranslated ? 6 : 1;   // the translated arm maps positions through 6 segments per record
    E.offbuf.ensure(((size_t)nrec + 1) * 8);
    E.grpbuf.ensure((size_t)nrec * per * 4);
    HIP_CHECK(hipMemcpyAsync(E.offbuf.ptr, off, ((size_t)nrec + 1) * 8, hipMemcpyHostToDevice, s));
    Workspace ws(s);
    uint32_t* d_groups = ws.take<uint32_t>(groups && per > 1 ? nrec : 1);
    uint32_t* d_err = ws.take<uint32_t>(1);
    if (groups && per == 1) {
      HIP_CHECK(hipMemcpyAsync(E.grpbuf.ptr, groups, (size_t)nrec * 4, hipMemcpyHostToDevice, s));
    } else {
      if (groups) HIP_CHECK(hipMemcpyAsync(d_groups, groups, (size_t)nrec * 4, hipMemcpyHostToDevice, s));
      launch_index_build_groups(groups ? d_groups : nullptr, (uint64_t)nrec * per, per, E.grpbuf.as<uint32_t>(), s);
    }
    HIP_CHECK(hipMemsetAsync(d_err, 0xff, 4, s));
    HIP_CHECK(hipStreamSynchronize(s));   // (the caller's arrays, or the vectors above, were read by the uploads)
    SeqBatch b;
    b.seq = seq_dev; b.len = total_len; b.starts = E.offbuf.as<uint64_t>(); b.nrec = nrec; b.vend0 = total_len;
    BatchSource src(kind, like, b, off, s);
    const uint64_t P = src.positions();

    // Folds: stretches of the position space expected to leave `budget` candidates, as the grouped path cuts its chunks
    // (at most 2^30: one chunk of candidates holds fewer than 2^31 with its head-room)
    const long double frac = ((long double)like.max_hash + 1.0L) / 18446744073709551616.0L;
    const long double want = (long double)std::min<uint64_t>(std::max<uint64_t>(g_index_build_budget, 1), 1ull << 30) / frac;
    const uint64_t CH = want > 4.0e12L ? (uint64_t)4e12 : std::max<uint64_t>((uint64_t)want, 1);
    std::vector<Runs> folds;
    uint64_t held = 0;
    for (uint64_t lo = 0; lo < P; lo += CH) {
      const uint64_t hi = std::min(P, lo + CH);
      const uint64_t nc = E.run_chunk(src.ref(), lo, hi, like.max_hash, true, s);
      if (nc == 0) continue;
      dev.count("index_build_fold");
      // (hash, position) -> (hash, group); sort by hash, then stably by group: (group, hash) order
      launch_pos_to_group(E.cand_pos[0].as<uint64_t>(), nc, src.pos_table, src.pos_entries, E.grpbuf.as<uint32_t>(), s, 0);
      const int c1 = radix_sort_u64(E.cand_hash[0].as<uint64_t>(), E.cand_hash[1].as<uint64_t>(), E.cand_pos[0].as<uint64_t>(),
                                    E.cand_pos[1].as<uint64_t>(), nc, dev.scratch, s);
      const int c2 = radix_sort_u64(E.cand_pos[c1].as<uint64_t>(), E.cand_pos[c1 ^ 1].as<uint64_t>(), E.cand_hash[c1].as<uint64_t>(),
                                    E.cand_hash[c1 ^ 1].as<uint64_t>(), nc, dev.scratch, s, 0, 8);
      const int cur = c1 ^ c2;
      Runs f = runs_of(E.cand_hash[cur].as<uint64_t>(), E.cand_pos[cur].as<uint64_t>(), nc, 0, d_err, dev, s);
      held += f.n;
      folds.push_back(std::move(f));
      if (held > kMaxPairs) {   // merged early: what is held stays below 2^32 elements, and the refusal is exact
        Runs m = merge_runs(folds, d_err, dev, s);
        if (m.n > kMaxPairs)
          refuse("the result would hold more than 2^31 - 1 (group, hash) pairs (" + std::to_string(m.n) + " so far); build it in pieces");
        held = m.n;
        folds.push_back(std::move(m));
      }
    }
    if (src.have_error) throw src.err;   // the translated arm's UTF-8 panic
    const bool merged = folds.size() > 1;
    if (merged) { Runs m = merge_runs(folds, d_err, dev, s); folds.push_back(std::move(m)); }
    uint32_t err = kBuildNoError;
    HIP_CHECK(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (err != kBuildNoError && has_abunds)
      refuse("group " + std::to_string(err) + " holds a hash seen in 2^32 or more windows; a sketch of an index keeps 32 bits per abundance");
    if (!folds.empty()) result = std::move(folds.back());
    folds.clear();
  }

  const uint64_t S = result.n;
  hashes.ensure(S * 8 + 8);   // (the padding of pack_sketches: the compare kernels read a little past the end)
  if (has_abunds) { abunds_dev.ensure(S * 4 + 4); abunds_resident = true; }
  offsets.ensure(h_offsets.size() * 8);
  nums.ensure((size_t)n * 4 + 4);
  HIP_CHECK(hipMemsetAsync(nums.ptr, 0, (size_t)n * 4 + 4, s));
  if (S) {
    HIP_CHECK(hipMemcpyAsync(hashes.ptr, result.hash, S * 8, hipMemcpyDeviceToDevice, s));
    launch_index_build_finish(result.pack, (uint32_t)S, G, offsets.as<uint64_t>(), has_abunds ? abunds_dev.as<uint32_t>() : nullptr,
                              dev, s);
    HIP_CHECK(hipMemcpyAsync(h_offsets.data(), offsets.ptr, h_offsets.size() * 8, hipMemcpyDeviceToHost, s));
  } else {
    HIP_CHECK(hipMemsetAsync(offsets.ptr, 0, h_offsets.size() * 8, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  if (h_offsets.front() != 0 || h_offsets.back() != S) throw_internal("index build: the group bounds do not span the runs");
  for (uint32_t g = 0; g < n; g++) max_len = std::max<uint32_t>(max_len, (uint32_t)(h_offsets[g + 1] - h_offsets[g]));
  dev.count("index_built");
  enroll();
}

void check_index_concat(ResidentIndex* const* parts, uint32_t n_parts) {
  if (n_parts && !parts) refuse_concat("parts is NULL");
  uint64_t nodes = 0;
  for (uint32_t p = 0; p < n_parts; p++) {
    if (!parts[p]) refuse_concat("parts[" + std::to_string(p) + "] is NULL");
    nodes += parts[p]->n;
  }
  if (nodes > 0xfffffffeull) refuse_concat("the parts hold " + std::to_string(nodes) + " nodes; an index takes at most 2^32 - 2");
}

ResidentIndex::ResidentIndex(ResidentIndex* const* parts, uint32_t n_parts) {
  check_index_concat(parts, n_parts);
  has_abunds = true;
  bool any_resident = false;
  uint64_t total = 0;
  h_offsets.assign(1, 0);
  for (uint32_t p = 0; p < n_parts; p++) {
    const ResidentIndex& P = *parts[p];
    const uint64_t base = P.h_offsets.front(), len = P.h_offsets.back() - base;
    params.insert(params.end(), P.params.begin(), P.params.end());
    h_nums.insert(h_nums.end(), P.h_nums.begin(), P.h_nums.end());
    for (uint32_t i = 0; i < P.n; i++) h_offsets.push_back(P.h_offsets[i + 1] - base + total);
    has_abunds &= P.has_abunds;
    any_resident |= P.has_abunds && len && (P.angular_ready || P.abunds_resident);
    total += len;
  }
  n = (uint32_t)params.size();
  for (uint32_t i = 0; i < n; i++) {
    const KmerMinHash &q = params[i], &q0 = params[0];
    uniform &= q.ksize == q0.ksize && q.molecule == q0.molecule && q.max_hash == q0.max_hash && q.seed == q0.seed;
    any_num |= q.num != 0;
    all_scaled &= q.num == 0 && q.max_hash != 0;
    max_len = std::max<uint32_t>(max_len, (uint32_t)(h_offsets[i + 1] - h_offsets[i]));
  }
  {
    auto& dev = Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    hashes.ensure(total * 8 + 8);
    offsets.ensure(h_offsets.size() * 8);
    nums.ensure((size_t)n * 4 + 4);
    HIP_CHECK(hipMemsetAsync(offsets.ptr, 0, 8, s));   // (an index without nodes: the one offset)
    if (has_abunds && any_resident) { abunds_dev.ensure(total * 4 + 4); abunds_resident = true; }
    if (has_abunds && !any_resident) h_abunds.reserve(total);
    uint64_t at = 0;
    uint32_t node = 0;
    for (uint32_t p = 0; p < n_parts; p++) {
      const ResidentIndex& P = *parts[p];
      const uint64_t base = P.h_offsets.front(), len = P.h_offsets.back() - base;
      if (len) HIP_CHECK(hipMemcpyAsync(hashes.as<uint64_t>() + at, P.hashes.as<uint64_t>() + base, len * 8, hipMemcpyDeviceToDevice, s));
      // offsets[node .. node + P.n] = the part's, moved by (at - base); the shared boundary is written twice with one value
      launch_index_build_rebase(P.offsets.as<uint64_t>(), (uint64_t)P.n + 1, at - base, offsets.as<uint64_t>() + node, s);
      if (P.n) HIP_CHECK(hipMemcpyAsync(nums.as<uint32_t>() + node, P.nums.ptr, (size_t)P.n * 4, hipMemcpyDeviceToDevice, s));
      if (has_abunds && len) {
        const bool on_device = P.angular_ready || P.abunds_resident;
        if (abunds_resident)
          HIP_CHECK(hipMemcpyAsync(abunds_dev.as<uint32_t>() + at, on_device ? (const void*)(P.abunds_dev.as<uint32_t>() + base) : (const void*)P.h_abunds.data(),
                                   len * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        else
          h_abunds.insert(h_abunds.end(), P.h_abunds.begin(), P.h_abunds.end());
        for (uint64_t w : P.wide_pos) wide_pos.push_back(w - base + at);
        if (P.wide_node != kAngularNoError) wide_node = std::min(wide_node, node + P.wide_node);
      }
      at += len;
      node += P.n;
    }
    HIP_CHECK(hipStreamSynchronize(s));
    dev.count("index_concat");
  }
  enroll();
}

}  // namespace smh
