// sigtext.cpp -- signature JSON written on the device: the host side of sigtext_kernels.hip.  The device
// counts the digits of every value; the host receives 16 bytes per node, builds the skeleton -- the few hundred bytes of a
// signature around its two arrays, with the one string writer the library has (sigjson.hpp's json_escape) -- and lays the
// text out with sigtext_core.hpp's walk; the device then writes the digits, the md5 of every node and the skeleton into place.
#include "sigtext.hpp"

#include <string>

#include "sigjson.hpp"
#include "sigtext_core.hpp"

namespace smh {

namespace {

[[noreturn]] void refuse(const std::string& what) { throw Error(kMsg, "sigtext: " + what); }

// the layout as the kernels take it: the skeleton's bytes one after another and where each run of them goes
struct PlaceSink {
  std::string skeleton;
  std::vector<uint64_t> piece_src, piece_dst, mins_at, abunds_at, md5_at, doc_offsets;
  uint64_t next_dst = ~0ull;   // where a piece must stand to continue the one in front of it
  void document(uint32_t, uint64_t at) { doc_offsets.push_back(at); }
  void piece(const char* bytes, uint64_t len, uint64_t at) {
    if (!len) return;
    if (at != next_dst) { piece_src.push_back(skeleton.size()); piece_dst.push_back(at); }
    skeleton.append(bytes, len);
    next_dst = at + len;
  }
  void mins(uint32_t v, uint64_t at) { mins_at[v] = at; }
  void abunds(uint32_t v, uint64_t at) { abunds_at[v] = at; }
  void md5(uint32_t v, uint64_t at) { md5_at[v] = at; }
};

std::string json_or_null(const char* const* strings, uint32_t v) {
  if (!strings || !strings[v]) return "null";
  std::string out;
  json_escape(out, strings[v]);
  return out;
}

template <class T> T* upload(Workspace& ws, const std::vector<T>& v, hipStream_t s) {
  T* d = ws.take<T>(v.size() + 1);
  if (!v.empty()) HIP_CHECK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
  return d;
}

std::vector<uint32_t> ksizes_of(const ResidentIndex& index) {
  std::vector<uint32_t> k(index.n);
  for (uint32_t v = 0; v < index.n; v++) k[v] = index.params[v].ksize;
  return k;
}

}  // namespace

void check_sigtext(const ResidentIndex& index, const uint32_t* doc_starts, uint32_t n_docs) {
  if (doc_starts) {
    if (doc_starts[0] != 0) refuse("doc_starts[0] is " + std::to_string(doc_starts[0]) + "; the documents begin at node 0");
    for (uint32_t d = 0; d < n_docs; d++)
      if (doc_starts[d] > doc_starts[d + 1])
        refuse("doc_starts[" + std::to_string(d + 1) + "] is " + std::to_string(doc_starts[d + 1]) + ", below doc_starts[" + std::to_string(d) +
               "] = " + std::to_string(doc_starts[d]) + "; the documents must ascend");
    if (doc_starts[n_docs] != index.n)
      refuse("doc_starts[" + std::to_string(n_docs) + "] is " + std::to_string(doc_starts[n_docs]) + "; the documents end at the index's " +
             std::to_string(index.n) + " nodes");
  }
  if (index.has_abunds && index.wide_node != kAngularNoError)
    refuse("node " + std::to_string(index.wide_node) + " holds an abundance of 2^32 or more, whose value the index no longer has");
}

void index_sigtext(SigText* out, ResidentIndex& index, const char* const* names, const char* const* filenames, const uint32_t* doc_starts,
                   uint32_t n_docs, Device& dev) {
  check_sigtext(index, doc_starts, n_docs);
  const uint32_t n = index.n;
  const uint64_t base = index.h_offsets.front(), total = index.h_offsets.back() - base;
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  Workspace ws(s);
  SigTextPass p;
  p.hashes = index.hashes.as<uint64_t>() + base;
  p.total = total;
  p.off = index.offsets.as<uint64_t>();
  p.n = n;
  // the abundances: read in place when they live in HBM, else uploaded for the call
  if (index.has_abunds) {
    if (index.angular_ready || index.abunds_resident) {
      p.abunds = index.abunds_dev.as<uint32_t>() + base;
    } else {
      uint32_t* ab = ws.take<uint32_t>(total);
      if (total) HIP_CHECK(hipMemcpyAsync(ab, index.h_abunds.data(), total * 4, hipMemcpyHostToDevice, s));
      p.abunds = ab;
    }
  }
  const uint64_t tiles = sigtext_tiles(total);
  p.tile_h = ws.take<uint64_t>(tiles + 1);
  p.node_h = ws.take<uint64_t>((size_t)n + 1);
  if (p.abunds) { p.tile_a = ws.take<uint64_t>(tiles + 1); p.node_a = ws.take<uint64_t>((size_t)n + 1); }
  if (n) launch_sigtext_measure(p, dev, s);   // (an index without nodes may hold no offsets)
  // the md5s need nothing of the layout: they run while the host lays the text out
  const std::vector<uint32_t> ksizes = ksizes_of(index);
  uint32_t* d_ksizes = upload(ws, ksizes, s);
  uint8_t* digests = ws.take<uint8_t>((size_t)n * 16);
  std::vector<uint64_t> node_h((size_t)n + 1, 0), node_a((size_t)n + 1, 0);
  if (n) HIP_CHECK(hipMemcpyAsync(node_h.data(), p.node_h, node_h.size() * 8, hipMemcpyDeviceToHost, s));
  if (n && p.abunds) HIP_CHECK(hipMemcpyAsync(node_a.data(), p.node_a, node_a.size() * 8, hipMemcpyDeviceToHost, s));
  launch_sigtext_md5(p.hashes, p.off, n, d_ksizes, digests, dev, s);
  // the skeleton, while the device works
  std::vector<sigtext::NodeText> nodes(n);
  for (uint32_t v = 0; v < n; v++) {
    const KmerMinHash& q = index.params[v];
    const sigtext::NodeParams np{q.num, q.ksize, q.seed, q.max_hash, molecule_name(q.molecule)};
    nodes[v] = sigtext::node_text(np, json_or_null(filenames, v), json_or_null(names, v), index.has_abunds);
  }
  HIP_CHECK(hipStreamSynchronize(s));
  std::vector<uint64_t> counts(n);
  for (uint32_t v = 0; v < n; v++) {
    counts[v] = index.h_offsets[v + 1] - index.h_offsets[v];
    // (what the layout trusts: a value has 1 .. 20 digits, an abundance 1 .. 10)
    const uint64_t h = node_h[v + 1] - node_h[v], a = node_a[v + 1] - node_a[v];
    if (node_h[v + 1] < node_h[v] || h < counts[v] || h > counts[v] * sigtext::kMaxDigits64 ||
        (p.abunds && (node_a[v + 1] < node_a[v] || a < counts[v] || a > counts[v] * sigtext::kMaxDigits32)))
      throw_internal("sigtext: the digit totals of node " + std::to_string(v) + " are out of range");
    node_h[v] = h;
    node_a[v] = a;
  }
  PlaceSink sink;
  sink.mins_at.assign(n, 0); sink.abunds_at.assign(n, 0); sink.md5_at.assign(n, 0);
  out->len = sigtext::walk_layout(n, doc_starts, n_docs, nodes.data(), node_h.data(), node_a.data(), counts.data(), index.has_abunds, sink);
  out->doc_offsets = std::move(sink.doc_offsets);
  nodes.clear(); nodes.shrink_to_fit();
  out->text = std::make_unique<PoolBlock>(out->len + 64);
  SigTextPlace w;
  w.skeleton_len = sink.skeleton.size();
  w.pieces = sink.piece_dst.size();
  sink.piece_src.push_back(sink.skeleton.size());
  uint8_t* skel = ws.take<uint8_t>(sink.skeleton.size() + 1);
  HIP_CHECK(hipMemcpyAsync(skel, sink.skeleton.data(), sink.skeleton.size(), hipMemcpyHostToDevice, s));
  w.skeleton = skel;
  w.piece_src = upload(ws, sink.piece_src, s);
  w.piece_dst = upload(ws, sink.piece_dst, s);
  w.mins_at = upload(ws, sink.mins_at, s);
  if (p.abunds) w.abunds_at = upload(ws, sink.abunds_at, s);
  w.md5_at = upload(ws, sink.md5_at, s);
  w.digests = digests;
  w.text = out->text->as<uint8_t>();
  w.text_len = out->len;
  launch_sigtext_emit(p, w, dev, s);
  HIP_CHECK(hipStreamSynchronize(s));   // (the uploads read `sink` until here)
  dev.count("index_sigtext");
}

void index_md5(ResidentIndex& index, uint8_t* out, Device& dev) {
  const uint32_t n = index.n;
  if (n == 0) return;
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  Workspace ws(s);
  const std::vector<uint32_t> ksizes = ksizes_of(index);
  uint32_t* d_ksizes = upload(ws, ksizes, s);
  uint8_t* digests = ws.take<uint8_t>((size_t)n * 16);
  launch_sigtext_md5(index.hashes.as<uint64_t>() + index.h_offsets.front(), index.offsets.as<uint64_t>(), n, d_ksizes, digests, dev, s);
  HIP_CHECK(hipMemcpyAsync(out, digests, (size_t)n * 16, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace smh
