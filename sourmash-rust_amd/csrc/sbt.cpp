// sbt.cpp -- Nodegraph (reference src/index/nodegraph.rs) on the host, its batched device forms, and the resident
// Sequence Bloom Tree (reference src/index/sbt.rs): load / build / save and the batched, level-synchronous find.
#include "sbt.hpp"

#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <unordered_map>

#include "kernels.hpp"

namespace smh {

void TableLayout::init(const std::vector<uint64_t>& tablesizes) {
  sizes = tablesizes;
  woff.assign(1, 0);
  magic.clear();
  for (uint64_t s : sizes) {
    if (s == 0) throw_panic("attempt to calculate the remainder with a divisor of zero");
    if (s >= (1ull << 32)) throw Error(kMsg, "nodegraph table sizes must be below 2^32");
    woff.push_back(woff.back() + (uint32_t)((s + 63) / 64));
    magic.push_back(~0ull / s);
  }
}

void DeviceLayout::upload(const TableLayout& L, hipStream_t s) {
  T = L.n_tables(); W = L.words();
  std::vector<uint8_t> h((size_t)T * 8 + (size_t)(T + 1) * 4 + (size_t)T * 4 + 16);
  uint64_t* m = (uint64_t*)h.data();
  uint32_t* wo = (uint32_t*)(h.data() + (size_t)T * 8);
  uint32_t* sz = wo + T + 1;
  for (uint32_t t = 0; t < T; t++) { m[t] = L.magic[t]; sz[t] = (uint32_t)L.sizes[t]; }
  for (uint32_t t = 0; t <= T; t++) wo[t] = L.woff[t];
  buf.ensure(h.size());
  HIP_CHECK(hipMemcpyAsync(buf.ptr, h.data(), h.size(), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));   // `h` is host staging
  magic = buf.as<uint64_t>();
  woff = (const uint32_t*)((uint8_t*)buf.ptr + (size_t)T * 8);
  sizes = woff + T + 1;
}

// ------------------------------------------------------------------ Nodegraph (host)

Nodegraph::Nodegraph(const std::vector<uint64_t>& tablesizes, uint32_t k) : ksize(k) {
  L.init(tablesizes);
  words.assign(L.words(), 0);
}

bool Nodegraph::count(uint64_t h) {
  bool is_new = false;
  for (uint32_t t = 0; t < L.n_tables(); t++) {
    const uint64_t b = h % L.sizes[t];
    uint64_t& w = words[L.woff[t] + (b >> 6)];
    if (!((w >> (b & 63)) & 1)) { w |= 1ull << (b & 63); occupied_bins++; is_new = true; }
  }
  if (is_new) unique_kmers++;
  return is_new;
}

uint32_t Nodegraph::get(uint64_t h) const {
  for (uint32_t t = 0; t < L.n_tables(); t++)
    if (!bit(t, h % L.sizes[t])) return 0;
  return 1;
}

void Nodegraph::update(const Nodegraph& o) {
  const uint32_t T = std::min(L.n_tables(), o.L.n_tables());   // zip
  for (uint32_t t = 0; t < T; t++) {
    const uint32_t nw = L.woff[t + 1] - L.woff[t], onw = o.L.woff[t + 1] - o.L.woff[t];
    for (uint32_t w = 0; w < onw; w++) {
      uint64_t v = o.words[o.L.woff[t] + w];
      if (!v) continue;
      // FixedBitSet::put panics on a bit past the table (the other graph's table is larger and has it set)
      const uint64_t hi_bit = (uint64_t)w * 64 + 63 - __builtin_clzll(v);
      if (w >= nw || hi_bit >= L.sizes[t]) throw_panic("put at index exceeds fixbitset size");
      words[L.woff[t] + w] |= v;
    }
  }
}

namespace {
// |A n B| and |A u B| of table t of a and table t of b (tables of different sizes: the union holds both)
void inter_union(const Nodegraph& a, const Nodegraph& b, uint32_t t, uint64_t* inter, uint64_t* uni) {
  const uint32_t na = a.L.woff[t + 1] - a.L.woff[t], nb = b.L.woff[t + 1] - b.L.woff[t];
  const uint64_t* A = a.words.data() + a.L.woff[t];
  const uint64_t* B = b.words.data() + b.L.woff[t];
  uint64_t i = 0, u = 0;
  for (uint32_t w = 0; w < std::max(na, nb); w++) {
    const uint64_t x = w < na ? A[w] : 0, y = w < nb ? B[w] : 0;
    i += __builtin_popcountll(x & y);
    u += __builtin_popcountll(x | y);
  }
  *inter = i; *uni = u;
}
}  // namespace

double Nodegraph::similarity(const Nodegraph& o) const {
  uint64_t in = 0, un = 0;
  for (uint32_t t = 0; t < std::min(L.n_tables(), o.L.n_tables()); t++) {
    uint64_t i, u;
    inter_union(*this, o, t, &i, &u);
    in += i; un += u;
  }
  return (double)in / (double)un;
}

double Nodegraph::containment(const Nodegraph& o) const {
  uint64_t in = 0, size = 0;
  for (uint32_t t = 0; t < std::min(L.n_tables(), o.L.n_tables()); t++) {
    uint64_t i, u;
    inter_union(*this, o, t, &i, &u);
    in += i;
  }
  for (uint64_t s : L.sizes) size += s;
  return (double)in / (double)size;
}

std::string nodegraph_bytes(const TableLayout& L, const uint64_t* words, uint32_t ksize, uint64_t n_occupied) {
  std::string out("OXLI");
  auto put = [&](uint64_t v, int bytes) { for (int i = 0; i < bytes; i++) out.push_back((char)((v >> (8 * i)) & 0xff)); };
  put(4, 1);   // version
  put(2, 1);   // ht_type
  put(ksize, 4);
  put(L.n_tables(), 1);
  put(n_occupied, 8);
  for (uint32_t t = 0; t < L.n_tables(); t++) {
    const uint64_t len = L.sizes[t];
    put(len, 8);
    // FixedBitSet's u32 blocks: full blocks as 4 bytes, the last partial one as ceil(rem / 8) bytes.  So a table whose
    // size is a multiple of 8 is written with len / 8 bytes, one less than from_reader reads (nodegraph.rs:107-125).
    const uint64_t* tw = words + L.woff[t];
    const uint64_t blocks = (len + 31) / 32;
    for (uint64_t i = 0; i < blocks; i++) {
      const uint32_t chunk = (uint32_t)(tw[i / 2] >> (32 * (i & 1)));
      if ((i + 1) * 32 <= len) put(chunk, 4);
      else {
        const uint64_t rem = len - i * 32;
        const uint64_t nbytes = rem % 8 ? rem / 8 + 1 : rem / 8;
        for (uint64_t p = 0; p < nbytes; p++) out.push_back((char)((chunk >> (8 * p)) & 0xff));
      }
    }
  }
  return out;
}

std::string Nodegraph::save() const { return nodegraph_bytes(L, words.data(), ksize, occupied_bins); }

Nodegraph Nodegraph::load(const char* data, size_t len) {
  size_t at = 0;
  auto need = [&](size_t n) {
    if (at + n > len) throw Error(kIo, "failed to fill whole buffer");
  };
  auto get = [&](int bytes) {
    need(bytes);
    uint64_t v = 0;
    for (int i = 0; i < bytes; i++) v |= (uint64_t)(uint8_t)data[at + i] << (8 * i);
    at += bytes;
    return v;
  };
  need(4);
  if (std::memcmp(data, "OXLI", 4) != 0) throw Error(kMsg, "nodegraph: bad signature (not an OXLI file)");
  at = 4;
  if (get(1) != 4) throw Error(kMsg, "nodegraph: unsupported file version");
  if (get(1) != 2) throw Error(kMsg, "nodegraph: not a nodegraph (table type)");
  const uint32_t ksize = (uint32_t)get(4);
  const uint32_t n_tables = (uint32_t)get(1);
  const uint64_t occupied = get(8);
  std::vector<uint64_t> sizes;
  std::vector<std::pair<size_t, uint64_t>> spans;   // (data offset, bytes) per table
  for (uint32_t t = 0; t < n_tables; t++) {
    const uint64_t ts = get(8);
    if (ts == 0 || ts >= (1ull << 32)) throw Error(kMsg, "nodegraph: table size out of range");
    const uint64_t nbytes = ts / 8 + 1;
    need(nbytes);
    sizes.push_back(ts);
    spans.emplace_back(at, nbytes);
    at += nbytes;
  }
  Nodegraph ng(sizes, ksize);
  for (uint32_t t = 0; t < n_tables; t++) {
    const uint8_t* p = (const uint8_t*)data + spans[t].first;
    for (uint64_t b = 0; b < spans[t].second; b++) {
      if (!p[b]) continue;
      for (int i = 0; i < 8; i++)
        if ((p[b] >> i) & 1) {
          const uint64_t bitno = b * 8 + i;
          if (bitno >= sizes[t]) throw_panic("insert at index exceeds fixbitset size");
          ng.words[ng.L.woff[t] + (bitno >> 6)] |= 1ull << (bitno & 63);
        }
    }
  }
  ng.occupied_bins = occupied;
  ng.unique_kmers = 0;   // khmer does not save it
  return ng;
}

namespace {
// the per-table bit offsets of a layout (count_many's min-index array) in device memory
void bit_bases(const TableLayout& L, std::vector<uint64_t>& base) {
  base.assign(L.n_tables() + 1, 0);
  for (uint32_t t = 0; t < L.n_tables(); t++) base[t + 1] = base[t] + L.sizes[t];
}
}  // namespace

void Nodegraph::count_many(const uint64_t* hashes, uint64_t n, uint8_t* out_new) {
  if (n == 0) return;
  if (n >= (1ull << 32)) throw Error(kMsg, "nodegraph count_many: at most 2^32 - 1 hashes per call");
  auto& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  DeviceLayout DL;
  DL.upload(L, s);
  std::vector<uint64_t> base;
  bit_bases(L, base);
  const uint32_t T = L.n_tables();
  DeviceBuffer dh, dw, dbins, dmin, dbase, dcnt, dout;
  dh.ensure(n * 8); dw.ensure((size_t)L.words() * 8 + 8); dbins.ensure(n * T * 4 + 4);
  dmin.ensure(base.back() * 4 + 4); dbase.ensure(base.size() * 8); dcnt.ensure(16); dout.ensure(n + 1);
  HIP_CHECK(hipMemcpyAsync(dh.ptr, hashes, n * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(dw.ptr, words.data(), (size_t)L.words() * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(dbase.ptr, base.data(), base.size() * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(dcnt.ptr, 0, 16, s));
  launch_sbt_bins(dh.as<uint64_t>(), n, DL, dbins.as<uint32_t>(), s);
  launch_ng_count_many(dh.as<uint64_t>(), n, DL, dw.as<uint64_t>(), dbins.as<uint32_t>(), dmin.as<uint32_t>(),
                       dbase.as<uint64_t>(), dcnt.as<unsigned long long>(), dout.as<uint8_t>(), s);
  uint64_t cnt[2];
  HIP_CHECK(hipMemcpyAsync(words.data(), dw.ptr, (size_t)L.words() * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(cnt, dcnt.ptr, 16, hipMemcpyDeviceToHost, s));
  if (out_new) HIP_CHECK(hipMemcpyAsync(out_new, dout.ptr, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  occupied_bins += cnt[0];
  unique_kmers += cnt[1];
}

void Nodegraph::get_many(const uint64_t* hashes, uint64_t n, uint8_t* out) const {
  if (n == 0) return;
  auto& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  DeviceLayout DL;
  DL.upload(L, s);
  DeviceBuffer dh, dw, dbins, dout;
  dh.ensure(n * 8); dw.ensure((size_t)L.words() * 8 + 8); dbins.ensure(n * L.n_tables() * 4 + 4); dout.ensure(n + 1);
  HIP_CHECK(hipMemcpyAsync(dh.ptr, hashes, n * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(dw.ptr, words.data(), (size_t)L.words() * 8, hipMemcpyHostToDevice, s));
  launch_sbt_bins(dh.as<uint64_t>(), n, DL, dbins.as<uint32_t>(), s);
  launch_ng_get_many(dbins.as<uint32_t>(), n, DL, dw.as<uint64_t>(), dout.as<uint8_t>(), s);
  HIP_CHECK(hipMemcpyAsync(out, dout.ptr, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// ------------------------------------------------------------------ the resident tree

namespace {
std::string dirname_of(const std::string& p) {
  const size_t k = p.find_last_of('/');
  if (k == std::string::npos) return ".";
  return k == 0 ? "/" : p.substr(0, k);
}
std::string basename_of(const std::string& p) {
  const size_t k = p.find_last_of('/');
  return k == std::string::npos ? p : p.substr(k + 1);
}
void write_file(const std::string& path, const std::string& bytes) {
  std::ofstream f(path, std::ios::binary | std::ios::trunc);
  if (!f) throw Error(kIo, "cannot create " + path);
  f.write(bytes.data(), (std::streamsize)bytes.size());
  if (!f) throw Error(kIo, "cannot write " + path);
}
uint64_t depth_of(uint64_t pos, uint32_t d) {
  uint64_t k = 0;
  while (pos) { pos = (pos - 1) / d; k++; }
  return k;
}
}  // namespace

SbtDev Sbt::dev_view() const {
  SbtDev t;
  t.tables = d_tables.as<uint64_t>();
  t.child = d_child.as<uint32_t>();
  t.min_n_below = d_mnb.as<uint64_t>();
  t.leaf_hashes = d_leaf_hashes.as<uint64_t>();
  t.leaf_off = d_leaf_off.as<uint64_t>();
  t.leaf_num = d_leaf_num.as<uint32_t>();
  t.d = d; t.W = L.words(); t.T = L.n_tables();
  t.woff = dl.woff;
  return t;
}

void Sbt::finalize(hipStream_t s) {
  if (d == 0) throw Error(kMsg, "sbt: d must be at least 1");
  const uint32_t N = n_nodes(), M = n_leaves();
  if (M >= kChildLeaf || N >= kChildLeaf) throw Error(kMsg, "sbt: too many nodes");
  std::unordered_map<uint64_t, uint32_t> nidx, lidx;
  for (uint32_t i = 0; i < N; i++) nidx[node_pos[i]] = i;
  for (uint32_t i = 0; i < M; i++) lidx[leaf_pos[i]] = i;
  // what SBT::find does at a position: the node map first, then the leaf map, else nothing (sbt.rs:158-170)
  auto at = [&](uint64_t pos) -> uint32_t {
    auto n = nidx.find(pos);
    if (n != nidx.end()) return n->second;
    auto l = lidx.find(pos);
    if (l != lidx.end()) return kChildLeaf | l->second;
    return kChildNone;
  };
  child.assign((size_t)N * d, kChildNone);
  for (uint32_t i = 0; i < N; i++)
    for (uint32_t c = 0; c < d; c++) {
      const uint64_t p = node_pos[i];
      if (p > (~0ull - c - 1) / d) continue;   // d * p + c + 1 overflows: no such position
      child[(size_t)i * d + c] = at((uint64_t)d * p + c + 1);
    }
  levels.clear();
  for (uint32_t i = 0; i < N;) {
    const uint64_t dep = depth_of(node_pos[i], d);
    uint32_t j = i;
    while (j < N && depth_of(node_pos[j], d) == dep) j++;
    levels.emplace_back(i, j);
    i = j;
  }
  // the order in which the reference's stack walk meets the leaves when every node passes: a walk that prunes subtrees
  // meets the leaves it reaches in the same relative order
  leaf_rank.assign(M, kChildNone);
  const uint32_t r0 = at(0);
  root_kind = r0 == kChildNone ? 0 : (r0 & kChildLeaf) ? 2 : 1;
  root_leaf = root_kind == 2 ? (r0 & ~kChildLeaf) : 0;
  {
    uint32_t rank = 0;
    std::vector<uint32_t> stack;
    if (r0 != kChildNone) stack.push_back(r0);
    while (!stack.empty()) {
      const uint32_t e = stack.back();
      stack.pop_back();
      if (e & kChildLeaf) { leaf_rank[e & ~kChildLeaf] = rank++; continue; }
      for (uint32_t c = 0; c < d; c++) {
        const uint32_t ch = child[(size_t)e * d + c];
        if (ch != kChildNone) stack.push_back(ch);
      }
    }
  }
  // device: layout, children, min_n_below, leaves (CSR, num)
  dl.upload(L, s);
  d_child.ensure(child.size() * 4 + 4);
  if (!child.empty()) HIP_CHECK(hipMemcpyAsync(d_child.ptr, child.data(), child.size() * 4, hipMemcpyHostToDevice, s));
  d_mnb.ensure((size_t)N * 8 + 8);
  if (N) HIP_CHECK(hipMemcpyAsync(d_mnb.ptr, min_n_below.data(), (size_t)N * 8, hipMemcpyHostToDevice, s));
  std::vector<const KmerMinHash*> v(M);
  std::vector<uint32_t> nums(M);
  for (uint32_t i = 0; i < M; i++) { v[i] = &leaf_sig[i].signatures[0]; nums[i] = v[i]->num; }
  SketchSet set;
  std::vector<uint64_t> hoff;
  Engine::get().pack_sketches(v, d_leaf_hashes, d_leaf_off, &set, &max_leaf_len, &hoff, s);
  d_leaf_num.ensure((size_t)M * 4 + 4);
  if (M) HIP_CHECK(hipMemcpyAsync(d_leaf_num.ptr, nums.data(), (size_t)M * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

Sbt* Sbt::load(const std::string& json_path) {
  const std::string text = read_file(json_path);
  const SbtJson js = sbt_json_from(text.data(), text.size());
  const std::string storage = dirname_of(json_path) + "/" + js.storage_path;
  std::unique_ptr<Sbt> t(new Sbt());
  t->d = js.d;
  t->factory_args = js.factory_args;
  std::vector<const SbtJsonEntry*> nodes, leaves;
  for (auto& e : js.nodes) nodes.push_back(&e);
  for (auto& e : js.leaves) leaves.push_back(&e);
  auto by_pos = [](const SbtJsonEntry* a, const SbtJsonEntry* b) { return a->pos < b->pos; };
  std::sort(nodes.begin(), nodes.end(), by_pos);
  std::sort(leaves.begin(), leaves.end(), by_pos);
  std::vector<uint64_t> words;
  for (size_t i = 0; i < nodes.size(); i++) {
    if (i && nodes[i]->pos == nodes[i - 1]->pos) throw Error(kSerdeError, "sbt: duplicate node position");
    const std::string raw = read_file(storage + "/" + nodes[i]->filename);
    Nodegraph ng = Nodegraph::load(raw.data(), raw.size());
    if (i == 0) { t->L = ng.L; t->ksize = ng.ksize; }
    else if (ng.L.sizes != t->L.sizes) throw Error(kMsg, "sbt: nodegraph " + nodes[i]->filename + " has other table sizes");
    words.insert(words.end(), ng.words.begin(), ng.words.end());
    t->node_pos.push_back(nodes[i]->pos);
    t->node_file.push_back(nodes[i]->filename);
    t->node_name.push_back(nodes[i]->name);
    t->min_n_below.push_back(nodes[i]->has_min_n_below ? nodes[i]->min_n_below : kNoMinNBelow);
    t->occupied.push_back(ng.occupied_bins);
  }
  for (size_t i = 0; i < leaves.size(); i++) {
    if (i && leaves[i]->pos == leaves[i - 1]->pos) throw Error(kSerdeError, "sbt: duplicate leaf position");
    const std::string raw = read_file(storage + "/" + leaves[i]->filename);
    std::vector<Signature> sigs = signatures_from_json(raw.data(), raw.size());
    // the leaf's data is the first sketch of the first signature (src/index.rs:95-106)
    if (sigs.empty() || sigs[0].signatures.empty()) throw_panic("index out of bounds: the len is 0 but the index is 0");
    sigs.resize(1);
    t->leaf_sig.push_back(std::move(sigs[0]));
    t->leaf_pos.push_back(leaves[i]->pos);
    t->leaf_file.push_back(leaves[i]->filename);
    t->leaf_name.push_back(leaves[i]->name);
  }
  auto& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  t->d_tables.ensure(words.size() * 8 + 8);
  if (!words.empty()) HIP_CHECK(hipMemcpyAsync(t->d_tables.ptr, words.data(), words.size() * 8, hipMemcpyHostToDevice, s));
  t->finalize(s);
  return t.release();
}

Sbt* Sbt::build(uint32_t d, const std::vector<uint64_t>& positions, const std::vector<const KmerMinHash*>& leaves,
                const std::vector<uint64_t>& tablesizes, uint32_t ksize) {
  if (d == 0) throw Error(kMsg, "sbt: d must be at least 1");
  const uint32_t M = (uint32_t)positions.size();
  std::unique_ptr<Sbt> t(new Sbt());
  t->d = d; t->ksize = ksize;
  t->L.init(tablesizes);
  t->factory_args = {ksize, tablesizes.empty() ? 0 : tablesizes[0], (uint64_t)tablesizes.size()};
  // leaves in position order
  std::vector<uint32_t> order(M);
  for (uint32_t i = 0; i < M; i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return positions[a] < positions[b]; });
  std::map<uint64_t, uint64_t> mnb;   // every ancestor position -> smallest leaf size below it
  std::map<std::string, int> used;
  for (uint32_t k = 0; k < M; k++) {
    const uint32_t i = order[k];
    if (k && positions[i] == positions[order[k - 1]]) throw Error(kMsg, "sbt build: two leaves at one position");
    leaves[i]->materialize();
    const uint64_t sz = leaves[i]->mins.size();
    for (uint64_t p = positions[i]; p;) {
      p = (p - 1) / d;
      auto it = mnb.find(p);
      if (it == mnb.end()) mnb[p] = sz; else it->second = std::min(it->second, sz);
    }
    Signature sig;
    std::string md5 = sketch_md5(*leaves[i]);
    sig.has_name = true; sig.name = md5;
    sig.has_filename = true; sig.filename = md5;
    sig.signatures.push_back(*leaves[i]);
    const std::string file = used[md5]++ ? md5 + "." + std::to_string(positions[i]) : md5;
    t->leaf_sig.push_back(std::move(sig));
    t->leaf_pos.push_back(positions[i]);
    t->leaf_file.push_back(file);
    t->leaf_name.push_back(md5);
  }
  for (uint64_t p : t->leaf_pos)
    if (mnb.count(p)) throw Error(kMsg, "sbt build: a leaf sits at the position of another leaf's ancestor");
  if (!mnb.empty() && tablesizes.empty()) throw Error(kMsg, "sbt build: a tree with internal nodes needs table sizes");
  for (auto& kv : mnb) {
    t->node_pos.push_back(kv.first);
    t->min_n_below.push_back(kv.second);
    t->node_file.push_back("internal." + std::to_string(kv.first));
    t->node_name.push_back("internal." + std::to_string(kv.first));
  }
  const uint32_t N = t->n_nodes();
  auto& dev = Device::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  const size_t tbytes = (size_t)N * t->L.words() * 8;
  t->d_tables.ensure(tbytes + 8);
  t->finalize(s);
  // leaf -> its parent's node index (kChildNone for a leaf at the root)
  std::vector<uint32_t> parent(M, kChildNone);
  {
    std::unordered_map<uint64_t, uint32_t> nidx;
    for (uint32_t i = 0; i < N; i++) nidx[t->node_pos[i]] = i;
    for (uint32_t i = 0; i < M; i++) if (t->leaf_pos[i]) parent[i] = nidx.at((t->leaf_pos[i] - 1) / d);
  }
  DeviceBuffer d_parent, d_occ;
  d_parent.ensure((size_t)M * 4 + 4);
  d_occ.ensure((size_t)N * 8 + 8);
  dev.prof_begin(s);
  if (tbytes) HIP_CHECK(hipMemsetAsync(t->d_tables.ptr, 0, tbytes, s));
  if (M) HIP_CHECK(hipMemcpyAsync(d_parent.ptr, parent.data(), (size_t)M * 4, hipMemcpyHostToDevice, s));
  const SbtDev view = t->dev_view();
  if (N) {
    launch_sbt_count_leaves(view, M, d_parent.as<uint32_t>(), t->dl, t->d_tables.as<uint64_t>(), s);
    for (size_t k = t->levels.size(); k-- > 0;)
      launch_sbt_or_level(view, t->levels[k].first, t->levels[k].second - t->levels[k].first, t->d_tables.as<uint64_t>(), s);
    if (t->L.n_tables()) launch_sbt_popcount(view, N, d_occ.as<uint64_t>(), s);
  }
  dev.prof_end("sbt_build", s);
  t->occupied.assign(N, 0);
  if (N && t->L.n_tables()) HIP_CHECK(hipMemcpyAsync(t->occupied.data(), d_occ.ptr, (size_t)N * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return t.release();
}

void Sbt::save(const std::string& json_path) const {
  std::string stem = basename_of(json_path);
  for (const char* suf : {".sbt.json", ".json"}) {
    const size_t n = strlen(suf);
    if (stem.size() > n && stem.compare(stem.size() - n, n, suf) == 0) { stem.resize(stem.size() - n); break; }
  }
  const std::string rel = ".sbt." + stem;
  const std::string dir = dirname_of(json_path) + "/" + rel;
  if (mkdir(dir.c_str(), 0755) != 0 && errno != EEXIST) throw Error(kIo, "cannot create " + dir);
  const uint32_t N = n_nodes(), W = L.words();
  std::vector<uint64_t> words((size_t)N * W);
  if (!words.empty()) {
    auto& dev = Device::get();
    std::lock_guard<std::recursive_mutex> lock(dev.mutex());
    hipStream_t s = dev.stream();
    HIP_CHECK(hipMemcpyAsync(words.data(), d_tables.ptr, words.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  for (uint32_t i = 0; i < N; i++)
    write_file(dir + "/" + node_file[i], nodegraph_bytes(L, words.data() + (size_t)i * W, ksize, occupied[i]));
  for (uint32_t i = 0; i < n_leaves(); i++) write_file(dir + "/" + leaf_file[i], signatures_to_json({&leaf_sig[i]}));
  auto q = [](const std::string& v) { std::string o; o.push_back('"'); for (char c : v) { if (c == '"' || c == '\\') o.push_back('\\'); o.push_back(c); } o.push_back('"'); return o; };
  std::string js = "{\"d\":" + std::to_string(d) + ",\"version\":5,\"storage\":{\"backend\":\"FSStorage\",\"args\":{\"path\":" + q(rel) +
                   "}},\"factory\":{\"class\":\"GraphFactory\",\"args\":[";
  for (size_t i = 0; i < factory_args.size(); i++) js += (i ? "," : "") + std::to_string(factory_args[i]);
  js += "]},\"nodes\":{";
  for (uint32_t i = 0; i < N; i++) {
    js += (i ? "," : "") + q(std::to_string(node_pos[i])) + ":{\"filename\":" + q(node_file[i]) + ",\"name\":" + q(node_name[i]) +
          ",\"metadata\":{";
    if (min_n_below[i] != kNoMinNBelow) js += "\"min_n_below\":" + std::to_string(min_n_below[i]);
    js += "}}";
  }
  js += "},\"leaves\":{";
  for (uint32_t i = 0; i < n_leaves(); i++)
    js += (i ? "," : "") + q(std::to_string(leaf_pos[i])) + ":{\"filename\":" + q(leaf_file[i]) + ",\"name\":" + q(leaf_name[i]) +
          ",\"metadata\":" + q(leaf_name[i]) + "}";
  js += "}}";
  write_file(json_path, js);
}

void Sbt::find_many(const std::vector<const KmerMinHash*>& queries, double threshold, bool containment,
                    std::vector<uint64_t>& offsets, std::vector<uint64_t>& positions) {
  const uint32_t nq = (uint32_t)queries.size(), M = n_leaves();
  offsets.assign((size_t)nq + 1, 0);
  positions.clear();
  if (nq == 0 || root_kind == 0) return;
  // leaf.check_compatible(query) for each distinct parameter set of the leaves: a query that fails one of them is only
  // an error if its walk reaches such a leaf (checked on the leaf-pair list below)
  std::vector<const KmerMinHash*> classes;
  std::vector<uint32_t> leaf_class(M);
  for (uint32_t i = 0; i < M; i++) {
    const KmerMinHash& a = leaf_sig[i].signatures[0];
    uint32_t c = 0;
    for (; c < classes.size(); c++) {
      const KmerMinHash& b = *classes[c];
      if (a.ksize == b.ksize && a.molecule == b.molecule && a.max_hash == b.max_hash && a.seed == b.seed) break;
    }
    if (c == classes.size()) classes.push_back(&a);
    leaf_class[i] = c;
  }
  std::vector<std::vector<uint32_t>> bad_code(nq);   // per query: the error code against each class (0 = compatible)
  std::vector<char> query_bad(nq, 0);
  for (uint32_t q = 0; q < nq; q++)
    for (uint32_t c = 0; c < classes.size(); c++) {
      uint32_t code = 0;
      try { classes[c]->check_compatible(*queries[q]); } catch (const Error& e) { code = e.code; }
      if (code) { if (bad_code[q].empty()) bad_code[q].assign(classes.size(), 0); bad_code[q][c] = code; query_bad[q] = 1; }
    }

  auto& dev = Device::get();
  auto& E = Engine::get();
  std::lock_guard<std::recursive_mutex> lock(dev.mutex());
  hipStream_t s = dev.stream();
  SketchSet qset;
  uint32_t max_q = 0;
  std::vector<uint64_t> qoff;
  E.pack_sketches(queries, w_qh, w_qoff, &qset, &max_q, &qoff, s);
  const uint32_t T = L.n_tables();
  w_bins.ensure((size_t)qoff.back() * T * 4 + 4);
  dev.prof_begin(s);
  if (n_nodes()) launch_sbt_bins(w_qh.as<uint64_t>(), qoff.back(), dl, w_bins.as<uint32_t>(), s);
  dev.prof_end("sbt_bins", s);
  SbtQueries Q;
  Q.off = w_qoff.as<uint64_t>(); Q.hashes = w_qh.as<uint64_t>(); Q.bins = w_bins.as<uint32_t>();
  const SbtDev view = dev_view();
  const bool lds = (size_t)L.words() * 8 <= 64 * 1024;

  // queries go in chunks so that the frontier and the leaf-pair list are bounded by their worst case
  uint32_t widest = 1;
  for (auto& lv : levels) widest = std::max(widest, lv.second - lv.first);
  const uint64_t per_query = std::max<uint64_t>(std::max<uint64_t>(widest, M), 1);
  const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nq, (8ull << 20) / per_query));
  std::vector<std::vector<uint32_t>> hits_of(nq);
  uint32_t err_query = kChildNone, err_code = 0;
  for (uint32_t c0 = 0; c0 < nq; c0 += chunk) {
    const uint32_t c1 = std::min(nq, c0 + chunk), nc = c1 - c0;
    const uint32_t lp_cap = (uint32_t)(nc * (uint64_t)std::max<uint32_t>(M, 1));
    const size_t fr_cap = (size_t)nc * widest;
    w_lp.ensure((size_t)lp_cap * 8 + 8);
    w_hits.ensure((size_t)lp_cap * 8 + 8);
    w_ctr.ensure(64);
    unsigned int* ctr = w_ctr.as<unsigned int>();   // [0] leaf pairs, [1] hits, [2] err query
    const unsigned int init[4] = {0, 0, kChildNone, 0};
    const uint32_t zero = 0;
    HIP_CHECK(hipMemcpyAsync(ctr, init, 16, hipMemcpyHostToDevice, s));
    std::vector<uint32_t> qids(nc);
    for (uint32_t k = 0; k < nc; k++) qids[k] = c0 + k;
    if (root_kind == 2) {
      std::vector<uint2> lp(nc);
      for (uint32_t k = 0; k < nc; k++) lp[k] = make_uint2(root_leaf, c0 + k);
      HIP_CHECK(hipMemcpyAsync(w_lp.ptr, lp.data(), (size_t)nc * 8, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(ctr, &nc, 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipStreamSynchronize(s));   // `lp` and `nc` are host staging on the stack
    } else {
      uint32_t widest_cnt = 1;
      for (auto& lv : levels) widest_cnt = std::max(widest_cnt, lv.second - lv.first);
      for (int b = 0; b < 2; b++) {
        w_cnt[b].ensure((size_t)widest_cnt * 4 + 4); w_off[b].ensure((size_t)widest_cnt * 4 + 4);
        w_q[b].ensure(fr_cap * 4 + 4);
      }
      w_fill.ensure((size_t)widest_cnt * 4 + 4);
      w_pass.ensure(fr_cap + 4);
      // level 0: every query of the chunk waits at the root
      HIP_CHECK(hipMemcpyAsync(w_cnt[0].ptr, &nc, 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(w_off[0].ptr, &zero, 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(w_q[0].ptr, qids.data(), (size_t)nc * 4, hipMemcpyHostToDevice, s));
      int cur = 0;
      for (size_t li = 0; li < levels.size(); li++) {
        const bool has_next = li + 1 < levels.size();
        SbtLevel lv;
        lv.n0 = levels[li].first; lv.nn = levels[li].second - levels[li].first;
        lv.cnt = w_cnt[cur].as<uint32_t>(); lv.off = w_off[cur].as<uint32_t>(); lv.q = w_q[cur].as<uint32_t>();
        lv.pass = w_pass.as<uint8_t>();
        lv.lp = w_lp.as<uint2>(); lv.lp_n = ctr; lv.lp_cap = lp_cap; lv.err_q = ctr + 2;
        const uint32_t nn_next = has_next ? levels[li + 1].second - levels[li + 1].first : 0;
        if (has_next) {
          lv.next_n0 = levels[li + 1].first;
          lv.next_cnt = w_cnt[cur ^ 1].as<uint32_t>(); lv.next_off = w_off[cur ^ 1].as<uint32_t>();
          lv.next_fill = w_fill.as<uint32_t>(); lv.next_q = w_q[cur ^ 1].as<uint32_t>();
          HIP_CHECK(hipMemsetAsync(lv.next_cnt, 0, (size_t)nn_next * 4, s));
          HIP_CHECK(hipMemsetAsync(lv.next_fill, 0, (size_t)nn_next * 4, s));
        } else {
          // no internal children exist below the last level; the kernel never touches next_*
          lv.next_cnt = w_fill.as<uint32_t>();
        }
        launch_sbt_nodes(view, Q, lv, threshold, containment, lds, dev, s);
        if (has_next) {
          HIP_CHECK(hipMemcpyAsync(w_off[cur ^ 1].ptr, w_cnt[cur ^ 1].ptr, (size_t)nn_next * 4, hipMemcpyDeviceToDevice, s));
          exclusive_scan_u32_dev(w_off[cur ^ 1].as<uint32_t>(), nn_next, nullptr, dev.scratch, s);
          launch_sbt_fill(view, lv, s);
        }
        cur ^= 1;
      }
    }
    launch_sbt_leaves(view, Q, w_lp.as<uint2>(), ctr, lp_cap, threshold, containment, max_leaf_len, max_q,
                      w_hits.as<unsigned long long>(), ctr + 1, dev, s);
    unsigned int got[4];
    HIP_CHECK(hipMemcpyAsync(got, ctr, 16, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (got[0] > lp_cap) throw_internal("sbt find: leaf-pair list overflow");
    std::vector<unsigned long long> hits(got[1]);
    if (got[1]) HIP_CHECK(hipMemcpyAsync(hits.data(), w_hits.ptr, (size_t)got[1] * 8, hipMemcpyDeviceToHost, s));
    bool chunk_bad = false;
    for (uint32_t q = c0; q < c1; q++) chunk_bad |= query_bad[q] != 0;
    std::vector<uint2> lp;
    if (chunk_bad) {
      lp.resize(got[0]);
      if (got[0]) HIP_CHECK(hipMemcpyAsync(lp.data(), w_lp.ptr, (size_t)got[0] * 8, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    if (got[2] != kChildNone && got[2] < err_query) { err_query = got[2]; err_code = kPanic; }
    if (chunk_bad) {
      // the first reached leaf, in walk order, that the query is incompatible with (the reference stops there)
      std::vector<uint32_t> first_rank(nc, kChildNone), first_code(nc, 0);
      for (const uint2& p : lp) {
        const uint32_t q = p.y;
        if (!query_bad[q]) continue;
        const uint32_t code = bad_code[q][leaf_class[p.x]];
        if (code && leaf_rank[p.x] < first_rank[q - c0]) { first_rank[q - c0] = leaf_rank[p.x]; first_code[q - c0] = code; }
      }
      for (uint32_t k = 0; k < nc; k++)
        if (first_code[k] && c0 + k < err_query) { err_query = c0 + k; err_code = first_code[k]; }
    }
    for (unsigned long long h : hits) hits_of[(uint32_t)(h >> 32)].push_back((uint32_t)h);
  }
  if (err_query != kChildNone) {
    if (err_code == kPanic) throw_panic("no entry found for key \"min_n_below\" (node metadata)");
    throw_mismatch(err_code);
  }
  for (uint32_t q = 0; q < nq; q++) {
    auto& v = hits_of[q];
    std::sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return leaf_rank[a] < leaf_rank[b]; });
    for (uint32_t leaf : v) positions.push_back(leaf_pos[leaf]);
    offsets[q + 1] = positions.size();
  }
}

}  // namespace smh
