// sigscan.cpp -- signature JSON read on the device: the host side of sigscan_kernels.hip.  The device cuts
// the text into number spans, their values and a skeleton; the host parses the skeleton -- a few hundred bytes per signature --
// with the one JSON parser the library has (sigjson.hpp) and keeps what every sketch says.  An index is then gathered from the
// values with device-to-device copies.
#include "sigscan.hpp"

#include <algorithm>
#include <cctype>

#include "index.hpp"
#include "sigjson.hpp"

namespace smh {

namespace {

std::string at_doc(uint64_t doc, uint64_t off) { return "document " + std::to_string(doc) + ", byte " + std::to_string(off) + ": "; }

}  // namespace

void parse_signatures(Signatures* sigs, const void* text_in, bool text_on_host, uint64_t len, const uint64_t* doc_offsets, uint32_t n_docs,
                      void* stream, Device& dev) {
  const uint64_t whole[2] = {0, len};
  if (!doc_offsets) { doc_offsets = whole; n_docs = 1; }
  for (uint32_t d = 0; d < n_docs; d++)
    if (doc_offsets[d] > doc_offsets[d + 1]) throw Error(kMsg, "signatures: doc_offsets must ascend (document " + std::to_string(d) + ")");
  // the documents tile the text: the scan enters byte 0 outside a string, so bytes that belong to no document would decide how
  // every later document is read
  if (doc_offsets[0] != 0 || doc_offsets[n_docs] != len)
    throw Error(kMsg, "signatures: doc_offsets must begin at 0 and end at the text's length " + std::to_string(len) + " (they span " +
                      std::to_string(doc_offsets[0]) + " .. " + std::to_string(doc_offsets[n_docs]) + ")");
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = text_on_host ? dev.stream() : dev.user_stream(stream);
  Workspace ws(s);
  const uint8_t* text = static_cast<const uint8_t*>(text_in);
  if (text_on_host) {
    uint8_t* up = ws.take<uint8_t>(len + 64);
    if (len) HIP_CHECK(hipMemcpyAsync(up, text_in, len, hipMemcpyHostToDevice, s));
    text = up;
  }
  std::string skeleton;
  std::vector<SigSpanDev> rows;
  SigTotals tot{0, 0, 0, sigscan::kOut, 0};
  if (len) {
    void* scan = ws.take<uint8_t>(sigscan_workspace_bytes(text, len));
    SigTotals* totals_dev = ws.take<SigTotals>(1);
    launch_sigscan_scan(text, len, scan, totals_dev, dev, s);
    HIP_CHECK(hipMemcpyAsync(&tot, totals_dev, sizeof tot, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (tot.skeleton > len || tot.spans > len || tot.tokens > len) throw_internal("sigscan: more skeleton bytes, spans or tokens than text");
    sigs->values = std::make_unique<PoolBlock>(tot.tokens * 8 + 64);
    uint8_t* skel_dev = ws.take<uint8_t>(tot.skeleton + 64);
    SigSpanDev* rows_dev = ws.take<SigSpanDev>(tot.spans + 1);
    HIP_CHECK(hipMemsetAsync(rows_dev, 0xff, (tot.spans + 1) * sizeof(SigSpanDev), s));
    launch_sigscan_compact(text, len, scan, tot, skel_dev, rows_dev, sigs->values->as<uint64_t>(), dev, s);
    skeleton.resize(tot.skeleton);
    rows.resize(tot.spans);
    if (tot.skeleton) HIP_CHECK(hipMemcpyAsync(&skeleton[0], skel_dev, tot.skeleton, hipMemcpyDeviceToHost, s));
    if (tot.spans) HIP_CHECK(hipMemcpyAsync(rows.data(), rows_dev, tot.spans * sizeof(SigSpanDev), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  sigs->n_tokens = tot.tokens;
  // the span table
  const uint64_t ns = rows.size();
  sigs->spans.resize(ns);
  for (uint64_t k = 0; k < ns; k++) {
    SigSpanDev r = rows[k];
    if (r.end == sigscan::kNoOffset) {   // the text ends inside the span: only the last one can
      if (k + 1 != ns || tot.final_state < sigscan::kSpanNone) throw_internal("sigscan: a span without an end");
      r.end = len; r.end_token = tot.tokens; r.last_state = tot.final_state;
    }
    if (r.start > r.end || r.end > len || r.first_token > r.end_token || r.end_token > tot.tokens || (k && r.start <= rows[k - 1].start))
      throw_internal("sigscan: a span out of order");
    sigscan::SpanRow& o = sigs->spans[k];
    o.start = r.start; o.end = r.end; o.first_token = r.first_token; o.n_tokens = r.end_token - r.first_token;
    o.last_state = r.last_state;
    o.status = sigscan::span_status(r.bad_syntax, r.overflow, r.last_state, &o.bad_off);
  }
  const auto& spans = sigs->spans;
  const std::vector<uint64_t> removed = removed_prefix(spans);
  for (uint32_t d = 0; d < n_docs; d++) {
    const DocSlice slice = slice_document(spans, removed, doc_offsets[d], doc_offsets[d + 1]);
    const Holes& holes = slice.holes;
    const uint64_t first = slice.first_span, kb = slice.skel_begin, ke = slice.skel_end;
    if (ke > skeleton.size() || kb > ke) throw_internal("sigscan: a document outside the skeleton");
    try {
      JVal root;
      parse_document(skeleton.data() + kb, ke - kb, &holes, &root);
      std::vector<SigEntry> sketches;
      walk_document(root, &holes,
                    [&](size_t i, size_t k, const SketchFields& f) {
                      SigEntry en;
                      en.document = d; en.signature = (uint32_t)i; en.sketch = (uint32_t)k;
                      en.md5sum = f.md5sum; en.num = f.num; en.ksize = f.ksize; en.seed = f.seed; en.max_hash = f.max_hash;
                      en.molecule = f.molecule; en.has_abunds = f.has_abunds;
                      en.mins_span = first + (uint64_t)f.mins->span;
                      en.n_mins = spans[en.mins_span].n_tokens;
                      if (f.has_abunds) { en.abunds_span = first + (uint64_t)f.abunds->span; en.n_abunds = spans[en.abunds_span].n_tokens; }
                      sketches.push_back(std::move(en));
                    },
                    [&](size_t, const SignatureFields& f) {
                      for (SigEntry& en : sketches) {
                        en.name = f.name; en.has_name = f.has_name; en.filename = f.filename; en.has_filename = f.has_filename;
                        en.license = f.license; en.klass = f.klass;
                        sigs->entries.push_back(std::move(en));
                      }
                      sketches.clear();
                    });
    } catch (const JsonError& err) {
      if (err.split_float)
        throw Error(kMsg, "signatures: " + at_doc(d, err.at) + err.message + " is not read on this route (a float split in two); load the file with load_signatures");
      throw Error(kSerdeError, at_doc(d, err.at) + err.message);
    }
  }
  if (sigs->entries.size() > 0xfffffffeull) throw Error(kMsg, "signatures: more than 2^32 - 2 sketches in one text");
  dev.count("signatures_parsed");
}

std::vector<uint32_t> signatures_filter(const Signatures& sigs, size_t ksize, const char* moltype) {
  std::string mt;
  if (moltype) for (const char* c = moltype; *c; c++) mt.push_back((char)tolower((unsigned char)*c));
  std::vector<uint32_t> ids;
  for (size_t i = 0; i < sigs.entries.size(); i++) {
    const SigEntry& e = sigs.entries[i];
    if (!(ksize == 0 || ksize == (size_t)e.ksize)) continue;
    if (moltype && !((mt == "dna" && e.molecule == kMoleculeDNA) || (mt == "protein" && e.molecule == kMoleculeProtein) ||
                     (mt == "dayhoff" && e.molecule == kMoleculeDayhoff) || (mt == "hp" && e.molecule == kMoleculeHp))) continue;
    ids.push_back((uint32_t)i);
  }
  return ids;
}

ResidentIndex::ResidentIndex(const Signatures& S, const uint32_t* ids, uint32_t n_ids) {
  const uint32_t n_entries = (uint32_t)S.entries.size();
  if (!ids) n_ids = n_entries;
  for (uint32_t j = 0; ids && j < n_ids; j++)
    if (ids[j] >= n_entries)
      throw Error(kMsg, "index from signatures: ids[" + std::to_string(j) + "] is " + std::to_string(ids[j]) + "; the text has " +
                        std::to_string(n_entries) + " sketches");
  if (n_ids > 0xfffffffeu) throw Error(kMsg, "index from signatures: the ids name " + std::to_string(n_ids) + " sketches; an index takes at most 2^32 - 2");
  n = n_ids;
  h_nums.resize(n);
  h_offsets.assign((size_t)n + 1, 0);
  std::vector<uint64_t> src((size_t)n + 1, 0), asrc((size_t)n + 1, 0);   // where node j's hashes / abundances begin in the values
  has_abunds = true;
  for (uint32_t j = 0; j < n; j++) {
    const SigEntry& e = S.entries[ids ? ids[j] : j];
    if (e.n_mins > 0xfffffffeull) throw Error(kMsg, "index from signatures: node " + std::to_string(j) + " holds " + std::to_string(e.n_mins) + " hashes; a node takes fewer than 2^32 - 1");
    h_nums[j] = e.num;
    KmerMinHash p(e.num, e.ksize, (Molecule)e.molecule, e.seed, e.max_hash, false);
    params.push_back(p);
    const KmerMinHash& p0 = params[0];
    uniform &= p.ksize == p0.ksize && p.molecule == p0.molecule && p.max_hash == p0.max_hash && p.seed == p0.seed;
    any_num |= p.num != 0;
    all_scaled &= p.num == 0 && p.max_hash != 0;
    has_abunds &= e.has_abunds && e.n_abunds == e.n_mins;
    src[j] = S.spans[e.mins_span].first_token;
    if (e.has_abunds) asrc[j] = S.spans[e.abunds_span].first_token;
    h_offsets[j + 1] = h_offsets[j] + e.n_mins;
    max_len = std::max<uint32_t>(max_len, (uint32_t)e.n_mins);
  }
  const uint64_t total = h_offsets.back();
  {
    auto& dev = Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    hashes.ensure(total * 8 + 8);   // (the padding of pack_sketches: the compare kernels read a little past the end)
    offsets.ensure(h_offsets.size() * 8);
    nums.ensure((size_t)n * 4 + 4);
    if (has_abunds) abunds_dev.ensure(total * 4 + 4);
    Workspace ws(s);
    uint64_t* d_src = ws.take<uint64_t>(src.size());
    uint64_t* d_asrc = ws.take<uint64_t>(asrc.size());
    unsigned long long* words = ws.take<unsigned long long>(2);   // the lowest unsorted place; the abundances of 2^32 or more
    unsigned long long got[2] = {~0ull, 0};
    HIP_CHECK(hipMemcpyAsync(d_src, src.data(), src.size() * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_asrc, asrc.data(), asrc.size() * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(words, got, 16, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(offsets.ptr, h_offsets.data(), h_offsets.size() * 8, hipMemcpyHostToDevice, s));
    if (n) HIP_CHECK(hipMemcpyAsync(nums.ptr, h_nums.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    launch_downsample_copy(S.values_dev(), nullptr, d_src, offsets.as<uint64_t>(), n, total, hashes.as<uint64_t>(), nullptr, dev, s);
    dev.prof_begin(s);
    launch_sigscan_gather_check(hashes.as<uint64_t>(), offsets.as<uint64_t>(), n, total, S.values_dev(), d_asrc,
                                has_abunds ? abunds_dev.as<uint32_t>() : nullptr, words, words + 1, nullptr, 0, dev, s);
    dev.prof_end("sigscan_gather", s);
    HIP_CHECK(hipMemcpyAsync(got, words, 16, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (got[0] != ~0ull) {
      const uint32_t node = (uint32_t)(got[0] >> 32), pos = (uint32_t)got[0];
      throw Error(kMsg, "index from signatures: node " + std::to_string(node) + " (sketch " + std::to_string(ids ? ids[node] : node) +
                        " of the text): the hash at position " + std::to_string(pos) +
                        " is not above the one in front of it; the hashes of a sketch must be strictly ascending");
    }
    if (got[1]) {   // few: their places, found by the same pass run again, in order
      const uint64_t nw = got[1];
      uint64_t* d_wide = ws.take<uint64_t>(nw);
      HIP_CHECK(hipMemsetAsync(words + 1, 0, 8, s));
      launch_sigscan_gather_check(hashes.as<uint64_t>(), offsets.as<uint64_t>(), n, total, S.values_dev(), d_asrc, abunds_dev.as<uint32_t>(),
                                  words, words + 1, d_wide, nw, dev, s);
      wide_pos.resize(nw);
      HIP_CHECK(hipMemcpyAsync(wide_pos.data(), d_wide, nw * 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      std::sort(wide_pos.begin(), wide_pos.end());
      wide_node = (uint32_t)(std::upper_bound(h_offsets.begin(), h_offsets.end(), wide_pos.front()) - h_offsets.begin() - 1);
    }
    abunds_resident = has_abunds;
    dev.count("index_from_signatures");
  }
  enroll();
}

}  // namespace smh
