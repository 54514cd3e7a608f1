// sbt.hpp -- Nodegraph (reference src/index/nodegraph.rs) and the resident Sequence Bloom Tree (reference
// src/index/sbt.rs): host objects and the launch interfaces of sbt_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "device.hpp"
#include "minhash.hpp"
#include "signature.hpp"

namespace smh {

// Table layout shared by the host Nodegraph, its device copy and every node of a tree: table t is words
// [woff[t], woff[t + 1]) of 64-bit words, bit b of the table = bit (b & 63) of word woff[t] + (b >> 6).
struct TableLayout {
  std::vector<uint64_t> sizes;   // bits per table, 1 .. 2^32 - 1
  std::vector<uint32_t> woff;    // n_tables + 1 word offsets
  std::vector<uint64_t> magic;   // floor((2^64 - 1) / size): the device modulo (sbt_kernels.hip fastmod)
  void init(const std::vector<uint64_t>& tablesizes);   // throws on a size of 0 or >= 2^32
  uint32_t words() const { return woff.empty() ? 0 : woff.back(); }
  uint32_t n_tables() const { return (uint32_t)sizes.size(); }
};

// The layout's per-table arrays in device memory (sizes as u32, word offsets, magic numbers)
struct DeviceLayout {
  DeviceBuffer buf;
  const uint32_t* sizes = nullptr;
  const uint32_t* woff = nullptr;
  const uint64_t* magic = nullptr;
  uint32_t T = 0, W = 0;
  void upload(const TableLayout& L, hipStream_t s);
};

struct Nodegraph {
  TableLayout L;
  std::vector<uint64_t> words;
  uint32_t ksize = 0;
  uint64_t occupied_bins = 0;
  uint64_t unique_kmers = 0;

  Nodegraph(const std::vector<uint64_t>& tablesizes, uint32_t ksize);
  bool count(uint64_t h);                 // nodegraph.rs:34-49
  uint32_t get(uint64_t h) const;         // 51-59
  void update(const Nodegraph& other);    // 62-89: OR, counters untouched
  double similarity(const Nodegraph& other) const;    // sum |A n B| / sum |A u B| over zipped tables
  double containment(const Nodegraph& other) const;   // sum |A n B| / sum of this graph's table sizes (199-224)
  std::string save() const;               // 97-129 (short last table when size % 8 == 0, as the reference)
  static Nodegraph load(const char* data, size_t len);   // 131-179, errors instead of asserts
  bool bit(uint32_t t, uint64_t b) const { return (words[L.woff[t] + (b >> 6)] >> (b & 63)) & 1; }
  // batched device forms
  void count_many(const uint64_t* hashes, uint64_t n, uint8_t* out_new);
  void get_many(const uint64_t* hashes, uint64_t n, uint8_t* out) const;
};
// the OXLI byte stream of one table set (header fields given): what Nodegraph::save writes
std::string nodegraph_bytes(const TableLayout& L, const uint64_t* words, uint32_t ksize, uint64_t n_occupied);

// ---- sbt_kernels.hip ----
// bins[i * T + t] = hashes[i] % sizes[t]
void launch_sbt_bins(const uint64_t* hashes, uint64_t n, const DeviceLayout& L, uint32_t* bins, hipStream_t s);
// Nodegraph::count over hashes[0 .. n) in array order on tables `words`: counters (occ, uniq: device u64) and out_new
// (nullable); minidx: one u32 per bit of all tables (work space)
void launch_ng_count_many(const uint64_t* hashes, uint64_t n, const DeviceLayout& L, uint64_t* words, const uint32_t* bins,
                          uint32_t* minidx, const uint64_t* bit_base, unsigned long long* counters, uint8_t* out_new, hipStream_t s);
void launch_ng_get_many(const uint32_t* bins, uint64_t n, const DeviceLayout& L, const uint64_t* words, uint8_t* out, hipStream_t s);

// The resident tree as the walk kernels see it.  Internal nodes are numbered in position order (= level order);
// child[i * d + c] encodes child c of node i: kChildNone, an internal node index, or kChildLeaf | leaf index.
constexpr uint32_t kChildNone = 0xffffffffu;
constexpr uint32_t kChildLeaf = 0x80000000u;
constexpr uint64_t kNoMinNBelow = ~0ull;
struct SbtDev {
  const uint64_t* tables = nullptr;    // n_nodes x W words
  const uint32_t* child = nullptr;     // n_nodes x d
  const uint64_t* min_n_below = nullptr;
  const uint64_t* leaf_hashes = nullptr;   // CSR
  const uint64_t* leaf_off = nullptr;
  const uint32_t* leaf_num = nullptr;
  uint32_t d = 2, W = 0, T = 0;
  const uint32_t* woff = nullptr;
};
// The query batch: CSR hashes and their bins (T per hash).
struct SbtQueries {
  const uint64_t* off = nullptr;
  const uint64_t* hashes = nullptr;
  const uint32_t* bins = nullptr;
};
// One level of the walk: nodes [n0, n0 + nn); the queries waiting at node n0 + g are q[off[g] .. off[g] + cnt[g]).
// Passing pairs count their internal children into next_cnt (indexed from next_n0) and append their leaf children to
// the leaf-pair list (lp, *lp_n, capacity lp_cap; *lp_n keeps counting past it).  *err_q = the smallest query that
// reached a node without min_n_below in similarity mode.
struct SbtLevel {
  uint32_t n0 = 0, nn = 0, next_n0 = 0;
  const uint32_t* cnt = nullptr;
  const uint32_t* off = nullptr;
  const uint32_t* q = nullptr;
  uint8_t* pass = nullptr;
  uint32_t* next_cnt = nullptr;
  uint32_t* next_fill = nullptr;
  const uint32_t* next_off = nullptr;
  uint32_t* next_q = nullptr;
  uint2* lp = nullptr;
  unsigned int* lp_n = nullptr;
  uint32_t lp_cap = 0;
  unsigned int* err_q = nullptr;
};
// lds: the node's tables fit in LDS (W * 8 bytes) -- staged once per node, else gathered from global memory
void launch_sbt_nodes(const SbtDev& t, const SbtQueries& q, const SbtLevel& lv, double threshold, bool containment,
                      bool lds, Device& dev, hipStream_t s);
void launch_sbt_fill(const SbtDev& t, const SbtLevel& lv, hipStream_t s);
// leaf pairs lp[0 .. min(*lp_n, cap)): compare(leaf, query) (similarity, leaf num truncates) or count_common / |leaf|;
// passing pairs are appended to hits as (query << 32 | leaf)
void launch_sbt_leaves(const SbtDev& t, const SbtQueries& q, const uint2* lp, const unsigned int* lp_n, uint32_t cap,
                       double threshold, bool containment, uint32_t max_leaf_len, uint32_t max_query_len,
                       unsigned long long* hits, unsigned int* hits_n, Device& dev, hipStream_t s);
// build: the leaves' hashes into their parents' tables (atomic OR), then children OR-ed into parents for the parents
// [p0, p0 + np) of one level; popcount of table 0 of every node -> occ
void launch_sbt_count_leaves(const SbtDev& t, uint32_t n_leaves, const uint32_t* leaf_parent, const DeviceLayout& L,
                             uint64_t* tables, hipStream_t s);
void launch_sbt_or_level(const SbtDev& t, uint32_t p0, uint32_t np, uint64_t* tables, hipStream_t s);
void launch_sbt_popcount(const SbtDev& t, uint32_t n_nodes, uint64_t* occ, hipStream_t s);

}  // namespace smh

namespace smh {

// The resident tree.  Internal nodes in position order (= level order, positions of one depth are contiguous), leaves
// in position order.  Tables, children, min_n_below and the leaves' CSR live in HBM from construction on.
class Sbt {
 public:
  static Sbt* load(const std::string& json_path);
  static Sbt* build(uint32_t d, const std::vector<uint64_t>& positions, const std::vector<const KmerMinHash*>& leaves,
                    const std::vector<uint64_t>& tablesizes, uint32_t ksize);
  void save(const std::string& json_path) const;
  // find for every query: offsets (n + 1) and positions, each list in the reference's walk order
  void find_many(const std::vector<const KmerMinHash*>& queries, double threshold, bool containment,
                 std::vector<uint64_t>& offsets, std::vector<uint64_t>& positions);

  uint32_t n_nodes() const { return (uint32_t)node_pos.size(); }
  uint32_t n_leaves() const { return (uint32_t)leaf_pos.size(); }
  const std::vector<uint64_t>& leaf_positions() const { return leaf_pos; }
  const KmerMinHash& leaf_sketch(uint32_t i) const { return leaf_sig[i].signatures[0]; }

 private:
  uint32_t d = 2;
  uint32_t ksize = 1;
  std::vector<uint64_t> factory_args;
  TableLayout L;
  std::vector<uint64_t> node_pos, min_n_below, occupied;
  std::vector<std::string> node_file, node_name;
  std::vector<uint64_t> leaf_pos;
  std::vector<Signature> leaf_sig;
  std::vector<std::string> leaf_file, leaf_name;
  // derived by finalize()
  std::vector<uint32_t> child;                           // n_nodes x d (see kChildNone / kChildLeaf)
  std::vector<std::pair<uint32_t, uint32_t>> levels;     // [first node, end) per depth
  std::vector<uint32_t> leaf_rank;                       // order of the leaf in the full walk (kChildNone: unreachable)
  int root_kind = 0;                                     // 0 none, 1 internal node 0, 2 leaf (index root_leaf)
  uint32_t root_leaf = 0;
  uint32_t max_leaf_len = 0;
  DeviceLayout dl;
  DeviceBuffer d_tables, d_child, d_mnb, d_leaf_hashes, d_leaf_off, d_leaf_num;
  // walk work space (grow-only)
  DeviceBuffer w_qh, w_qoff, w_bins, w_cnt[2], w_off[2], w_fill, w_q[2], w_pass, w_lp, w_hits, w_ctr;
  void finalize(hipStream_t s);                          // child table, levels, ranks, device upload of all but tables
  SbtDev dev_view() const;
};

}  // namespace smh
