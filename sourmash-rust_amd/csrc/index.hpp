// index.hpp -- a set of sketches resident in HBM and what is asked of it: block compares and gather (index.cpp), angular
// similarity on abundances (angular.cpp), matching records (match.cpp), gather of a batch (gather_many.cpp), taxonomic LCA
// (lca.cpp), the thresholded search of a batch (search_many.cpp), clustering (cluster.cpp) -- the four share query_batch.cpp
// -- collapsing by groups and the read-back (collapse.cpp), building one from records and concatenation (index_build.cpp),
// filtering its nodes and taking a subset of them (filter.cpp).
// The C boundary (ffi.cpp) only checks pointers and calls in here.
#pragma once
#include <cstdlib>
#include <functional>
#include <memory>

#include "minhash.hpp"

namespace smh {

struct SearchRowsOut;
struct Signatures;   // sigscan.hpp

struct ResidentIndex {
  DeviceBuffer hashes, offsets, nums;
  std::vector<uint64_t> h_offsets;
  std::vector<uint32_t> h_nums;
  std::vector<KmerMinHash> params;   // parameters only (mins cleared): check_compatible per node
  uint32_t max_len = 0, n = 0;
  // decided once for the whole set: every node has the parameters of node 0 (a sketch is then checked against that one
  // block), and whether any node is a bottom-`num` sketch
  bool uniform = true, any_num = false;
  bool all_scaled = true;   // every node has num == 0 and max_hash != 0: what a cut on the device requires
  // the dictionary of the resident set (dense ranks, components, frequent hashes), built by the first all-vs-all block of
  // the index with itself and kept: later ones skip the pre-pass (the nodes of an index never change)
  CollectionDict* dict = nullptr;
  uint32_t dict_split = 0;      // the frequent-hash setting the dictionary was built under
  // the hash directory: the sorted distinct hashes of all nodes and who holds each, built by the first
  // match() or gather_many() and kept like `dict`
  struct MatchDir* match_dir = nullptr;
  // angular similarity.  has_abunds: EVERY node tracks abundances and every abundance vector matches its
  // hashes; h_abunds then holds them narrowed to u32 (a copy, like the hashes) until the first angular call uploads them
  // and computes the norms -- an index nobody asks pays no HBM.  bad_node: the lowest node whose norm2 does not fit 64 bits.
  bool has_abunds = false;
  std::vector<uint32_t> h_abunds;
  uint32_t wide_node = kAngularNoError;   // the first node holding an abundance of 2^32 or more
  std::vector<uint64_t> wide_pos;         // where in the CSR those abundances are, ascending (few): a cut may drop them
  bool abunds_resident = false;           // a cut of a parent whose abundances were in HBM: abunds_dev holds them, h_abunds is empty
  bool angular_ready = false;
  uint32_t bad_node = kAngularNoError;
  DeviceBuffer abunds_dev, norm2_dev;
  std::vector<uint64_t> h_norm2;
  explicit ResidentIndex(const std::vector<const KmerMinHash*>& nodes);   // uploads the nodes
  // the parent's nodes cut at max_hash, built from the parent's device arrays: nothing comes to the host
  // but the kept lengths.  Refused (kMsg) unless every node is a scaled sketch and 0 < max_hash <= every node's max_hash.
  ResidentIndex(ResidentIndex& parent, uint64_t max_hash);
  // (collapse.cpp) the parent collapsed by groups (the rules: include/sourmash_amd.h, "Collapsing an index by groups"): node g
  // of the new index is the hashes that at least need_g members of group g hold, made from the parent's hash directory.
  // group: parent.n entries (nullable when the parent is empty), each below n_groups or kCollapseDrop; abund: CollapseAbund.
  // Every refusal is kMsg and comes before anything is built; the child carries no taxonomy (its nodes are not the parent's).
  ResidentIndex(ResidentIndex& parent, const uint32_t* group, uint32_t n_groups, uint32_t min_count, double min_fraction, uint32_t abund);
  // (index_build.cpp) Built from records on the device (the rules: include/sourmash_amd.h, "Building an index from records"):
  // node g holds what the records of group g leave in a fresh scaled sketch of `like`'s parameters.  input: BuildInput; seq_dev:
  // the batch in device memory, record r = [offsets[r], offsets[r + 1]) (host, n_records + 1 entries); groups: nullable (record r
  // is node r).  check_index_build is run first: every refusal that needs no device.  8 (n_groups + 1) bytes of offsets come
  // to the host, and two counts per fold; nothing proportional to the hashes crosses.
  ResidentIndex(const KmerMinHash& like, int input, const uint8_t* seq_dev, uint64_t total_len, const uint64_t* offsets,
                const uint32_t* groups, uint32_t n_records, uint32_t n_groups, hipStream_t s);
  // (index_build.cpp) The nodes of parts[0], then parts[1], ...: device-to-device copies, offsets rebased, no taxonomy,
  // dictionary or directory carried over.  The result owns its memory.
  ResidentIndex(ResidentIndex* const* parts, uint32_t n_parts);
  // (filter.cpp) The parent filtered (the rules: include/sourmash_amd.h, "Filtering an index"): the parent's nodes, in order and
  // with its parameters and taxonomy, each holding the hashes of the parent's node that pass the rule -- a verdict per
  // resident hash and an ordered compaction, made on the device.  operand: nullable under kFilterOperandNone; read where it
  // lives (a state in HBM is not brought to the host).  check_filter is run first, and the refusals that need the operand's
  // state (its abundances of 2^32 or more) come before anything is built.  8 (n + 1) bytes of offsets come to the host.  No
  // dictionary or directory is carried; the child's abundances, when it has them, are resident in HBM.
  ResidentIndex(ResidentIndex& parent, const KmerMinHash* operand, const FilterRule& rule);
  // (filter.cpp) Node j of the new index is node ids[j] of the parent, whole: any order, repeats allowed, n_ids may be 0.  Works on
  // every index (it only copies: device to device, balanced over the output by downsample_copy).  Carries the per-node
  // parameters and nums, the abundances wherever the parent has them (host or HBM), wide_pos / wide_node remapped and the
  // taxonomy with node_taxon permuted.  An id >= parent.n is refused (kMsg, the message names its position).
  ResidentIndex(ResidentIndex& parent, const uint32_t* ids, uint32_t n_ids);
  // (sigscan.cpp) Node j holds the `mins` of sketch ids[j] of a signature text read on the device (the rules:
  // include/sourmash_amd.h, "Signature JSON on the device"): any order, repeats allowed, ids null: every sketch in order.  The
  // hashes are copied device to device out of the text's values (downsample_copy, starts permuted); the parameters, uniform,
  // any_num, all_scaled, has_abunds, the narrowed abundances and wide_node / wide_pos are decided as the constructor from host
  // nodes decides them, so the result answers every call as smh_index_new(load_signatures(...)) does.  The abundances stay in
  // HBM (abunds_resident).  One refusal of its own (kMsg, nothing is built): a node whose hashes are not strictly ascending;
  // the lowest node and position are named.
  ResidentIndex(const Signatures& sigs, const uint32_t* ids, uint32_t n_ids);
  ~ResidentIndex();
  void enroll();   // into the registry of live indexes: the last step of every constructor
  // (collapse.cpp) the index as it is held: offsets (n + 1, from 0), hashes and abundances (offsets[n] each); any may be null.
  // Abundances come from the host copy or from HBM, wherever they live; asked of an index without them: kMsg.
  void read(uint64_t* offsets_out, uint64_t* hashes_out, uint32_t* abunds_out);
  void max_hash_range(uint64_t* lo, uint64_t* hi) const;   // over the nodes; 0, 0 when empty
  SketchSet set() const { return {hashes.as<uint64_t>(), offsets.as<uint64_t>(), n, h_offsets.data()}; }
  AngularSet angular_set() const {   // after angular_ensure
    return {hashes.as<uint64_t>(), abunds_dev.as<uint32_t>(), offsets.as<uint64_t>(), norm2_dev.as<uint64_t>(), n};
  }
  // check_compatible of every node with a sketch / with every node of another index.  A uniform index answers for all its
  // nodes with params[0]: the error depends only on the parameters, so its code and message are those of the full loop.
  void check_sketch(const KmerMinHash& mh, bool sketch_is_receiver = false) const;
  void check_index(const ResidentIndex& cols) const;
  // The one index-vs-index route: rows x cols into device memory.  An index against itself on the block route goes through
  // its cached dictionary (built here when missing or stale), everything else through launch_compare_block.
  static void compare_block(ResidentIndex& rows, ResidentIndex& cols, const CompareOut& dev_out, Device& dev, hipStream_t s);
  void drop_dict() { if (dict) { collection_free(dict); dict = nullptr; } }
  static void drop_all_dictionaries();   // of every live index (memory no other allocator can see)
  // outputs on the host, row-major; null = not wanted
  void compare(ResidentIndex& cols, double* jaccard, uint64_t* common, uint64_t* size, uint64_t* count_common, double* containment);
  // the index against one host sketch (n values each); q_is_row: the sketch is the row, its num cuts the union
  void vs_one(const KmerMinHash& q, bool q_is_row, double* jaccard, double* containment, uint64_t* count_common);
  uint32_t find(const KmerMinHash& query, double threshold, bool containment, uint32_t* out_indices);   // returns how many
  void most_common(const KmerMinHash& leaf, uint32_t* best_pos, uint64_t* best_common);
  uint32_t gather(const KmerMinHash& query, uint32_t threshold_common, GatherRow* rows, uint32_t rows_capacity, uint32_t* assigned,
                  Device& dev);
  // (match.cpp) The records of a batch against the index (the rules: include/sourmash_amd.h, "Matching records").  seq_dev:
  // the batch in device memory, record r = [offsets[r], offsets[r + 1]) (host, n + 1 ascending entries, the last at most
  // total_len).  rows: n entries.  hit_offsets (nullable: no hit list): n + 1 entries, *hit_hashes receives the list.
  void check_matchable() const;   // the refusals (kMsg): needs no device
  void match(const uint8_t* seq_dev, uint64_t total_len, const uint64_t* offsets, uint32_t n_records, MatchRow* rows,
             uint64_t* hit_offsets, std::vector<uint64_t>* hit_hashes, hipStream_t s);
  // The front half of match, shared with lca_records: the folds of a batch cut at record boundaries and per fold the grouped
  // fold's sequence up to the probe.  blank(a, e): records [a, e) are seen by no fold's kernels; tail(dir, fold): what the
  // caller does with a probed fold on `s` (the stream is waited for behind it and the fold's buffers go back).
  // check_match_batch: check_matchable and the offsets -- every refusal that needs no device, for callers to run in front of
  // their first write.
  struct MatchFold {
    uint32_t f0 = 0, nf = 0, nruns = 0;   // the fold's records [f0, f0 + nf) and its runs
    const uint64_t* run_hash = nullptr;   // nruns hashes
    MatchRow* rows = nullptr;             // nf rows: the four sums of the probe
    uint32_t* rec_first = nullptr;
    unsigned long long* rec_pairs = nullptr;
    uint32_t* rank = nullptr;             // nruns
    uint32_t* hit_flag = nullptr;         // nruns + 1 when the hits are wanted, else null
  };
  void check_match_batch(const uint64_t* offsets, uint32_t n_records, uint64_t total_len) const;
  void match_folds(const uint8_t* seq_dev, uint64_t total_len, const uint64_t* offsets, uint32_t n_records, bool want_hits, hipStream_t s,
                   const std::function<void(uint32_t, uint32_t)>& blank,
                   const std::function<void(const MatchDirectory&, const MatchFold&)>& tail);
  // The directory, built on the first call (counter match_directory_built).  An index of 2^31 or more hashes is refused
  // (kMsg, the message begins with `who`); check_directory_size is that refusal alone and needs no device.
  void check_directory_size(const char* who) const;
  MatchDirectory ensure_directory(const char* who, Device& dev, hipStream_t s);
  void drop_match_dir();
  // (query_batch.cpp) What the calls on the directory share in front of their kernels.  check_queries: every query as gather()
  // checks it -- a num sketch as query, a num sketch in the index, check_sketch -- the lowest failing query decides and the
  // message names it ("<who>: query q ..."); `can` is the operation's own phrase ("can be gathered").
  void check_queries(const char* who, const char* can, const KmerMinHash* const* queries, uint32_t n_queries) const;
  // the search kernels' view of the queries [a, b) of a CSR in device memory (self: SearchSelf); qoff, c and tile_rows are
  // the caller's blocks
  SearchChunk search_chunk(const uint64_t* q_hashes_dev, const uint64_t* q_offsets, uint32_t a, uint32_t b, uint32_t metric, double threshold,
                           uint32_t threshold_common, uint32_t self) const;
  // (gather_many.cpp) Gather of a batch of queries (the rules: include/sourmash_amd.h, smh_index_gather_many).  row_offsets
  // (n_queries + 1), *rows (row_offsets[n_queries] rows) and query_offsets (nullable, n_queries + 1) are written only when
  // the call succeeds; assigned (nullable, the queries' positions one after another) is filled chunk by chunk, after every
  // refusal the rules name.
  void gather_many(const KmerMinHash* const* queries, uint32_t n_queries, uint32_t threshold_common, uint32_t rows_capacity,
                   uint64_t* row_offsets, std::vector<GatherRow>* rows, uint64_t* query_offsets, uint32_t* assigned, Device& dev);
  // the CSR / device form: query q = q_hashes_dev[q_offsets[q] .. q_offsets[q + 1]); assigned counts from q_offsets[0]
  void gather_many_dev(const uint64_t* q_hashes_dev, const uint64_t* q_abunds_dev, const uint64_t* q_offsets, uint32_t n_queries,
                       uint32_t threshold_common, uint32_t rows_capacity, uint64_t* row_offsets, std::vector<GatherRow>* rows,
                       uint32_t* assigned, Device& dev, hipStream_t s);
  // (search_many.cpp) The (query, node) pairs over a threshold (the rules: include/sourmash_amd.h, smh_index_search_many).
  // Each returns the malloc'ed rows (one element at least; the caller frees them with free()), ordered by query, then node;
  // row_offsets (n_queries + 1, or n + 1 for search_self) is written only when the call succeeds.  metric: SearchMetric.
  SearchRow* search_many(const KmerMinHash* const* queries, uint32_t n_queries, uint32_t metric, double threshold,
                         uint32_t threshold_common, uint64_t* row_offsets, Device& dev);
  // the CSR / device form: query q = q_hashes_dev[q_offsets[q] .. q_offsets[q + 1]).  self (SearchSelf): the queries are this
  // index's nodes in order, and the diagonal (or everything up to it) is left out
  SearchRow* search_many_dev(const uint64_t* q_hashes_dev, const uint64_t* q_offsets, uint32_t n_queries, uint32_t metric, double threshold,
                             uint32_t threshold_common, uint32_t self, uint64_t* row_offsets, Device& dev, hipStream_t s);
  // the index against itself: the queries are read from the resident CSR in place
  SearchRow* search_self(uint32_t metric, double threshold, uint32_t threshold_common, bool upper_only, uint64_t* row_offsets, Device& dev);
  // What search_many_dev and nearest_dev are made of: the checks (`who` begins their messages), the early returns, the directory,
  // the chunks under search_many's budget (each counted as `chunk_counter`) and the rows' accounting.  Per chunk with a hash the
  // three blocks every search kernel reads (ck.qoff, uploaded; ck.c; ck.tile_rows) come from the chunk's workspace, then
  // tail(dir, ck, ws, out, starts) runs the kernels: it takes its further blocks from ws, makes room in `out` for the chunk's R
  // rows, brings them there, writes starts[1 .. ck.nq) -- where each later query's rows begin among them -- and returns R
  // with the stream waited for.
  using SearchChunkTail = std::function<uint32_t(const MatchDirectory&, const SearchChunk&, Workspace&, SearchRowsOut&, uint32_t*)>;
  SearchRow* search_chunks(const char* who, const char* chunk_counter, const uint64_t* q_hashes_dev, const uint64_t* q_offsets,
                           uint32_t n_queries, uint32_t metric, double threshold, uint32_t threshold_common, uint32_t self,
                           uint64_t* row_offsets, Device& dev, hipStream_t s, const SearchChunkTail& tail);
  // (nearest.cpp) Of those pairs, per query the best k by (value descending, node ascending) (the rules:
  // include/sourmash_amd.h, smh_index_nearest_many).  The three forms, the returned rows and row_offsets are search_many's,
  // but for the order of a query's rows; nearest_self leaves the diagonal out and nothing else.
  SearchRow* nearest_many(const KmerMinHash* const* queries, uint32_t n_queries, uint32_t k, uint32_t metric, double threshold,
                          uint32_t threshold_common, uint64_t* row_offsets, Device& dev);
  SearchRow* nearest_dev(const uint64_t* q_hashes_dev, const uint64_t* q_offsets, uint32_t n_queries, uint32_t k, uint32_t metric,
                         double threshold, uint32_t threshold_common, uint32_t self, uint64_t* row_offsets, Device& dev, hipStream_t s);
  SearchRow* nearest_self(uint32_t k, uint32_t metric, double threshold, uint32_t threshold_common, uint64_t* row_offsets, Device& dev);
  // (cluster.cpp) The clusters of the index under a symmetric metric (the rules: include/sourmash_amd.h, smh_index_cluster).
  // linkage: ClusterLinkage; scores (nullable, n entries): the priority, |S_v| when null.  cluster_out, representative (n
  // entries each), rep_common (nullable, n entries; greedy only) and *n_clusters are written only when the call succeeds.
  void cluster(uint32_t metric, double threshold, uint32_t threshold_common, uint32_t linkage, const uint32_t* scores, uint32_t* cluster_out,
               uint32_t* representative, uint32_t* rep_common, uint32_t* n_clusters, Device& dev);
  // (lca.cpp) Taxonomic LCA (the rules: include/sourmash_amd.h, "Taxonomic LCA").  The taxonomy is kept on the host
  // (tax_parent empty: none); the first device call uploads it and computes hash_taxon, one taxon per rank of the directory,
  // kept beside it in lca_dev (counter lca_table_built) and dropped with it, and by set_taxonomy.
  std::vector<uint32_t> tax_parent, tax_depth, node_taxon;
  struct LcaDev* lca_dev = nullptr;
  bool has_taxonomy() const { return !tax_parent.empty(); }
  void set_taxonomy(const uint32_t* parent, uint32_t n_taxa, const uint32_t* node_taxon_in, uint32_t n_nodes);   // host only
  void drop_lca_dev();
  struct LcaView { LcaTaxonomy tax; const uint32_t* hash_taxon = nullptr; };
  LcaView ensure_lca(const MatchDirectory& dir, Device& dev, hipStream_t s);
  void check_lca_sketches(const char* who) const;   // a taxonomy, and scaled nodes that agree in ksize, molecule, seed, max_hash
  // the counts of a batch of sketches / of a CSR in device memory: count_offsets (n_queries + 1), taxa / counts
  // (count_offsets[n_queries] pairs), query_offsets (nullable, n_queries + 1), hash_taxon (nullable, one per query position)
  void lca_many(const KmerMinHash* const* queries, uint32_t n_queries, uint64_t* count_offsets, std::vector<uint32_t>* taxa,
                std::vector<uint64_t>* counts, uint64_t* query_offsets, uint32_t* hash_taxon, Device& dev);
  void lca_many_dev(const uint64_t* q_hashes_dev, const uint64_t* q_offsets, uint32_t n_queries, uint64_t* count_offsets,
                    std::vector<uint32_t>* taxa, std::vector<uint64_t>* counts, uint32_t* hash_taxon, Device& dev, hipStream_t s);
  // the records of a batch classified (arguments as match's)
  void lca_records(const uint8_t* seq_dev, uint64_t total_len, const uint64_t* offsets, uint32_t n_records, LcaRow* rows, hipStream_t s);
  void angular_ensure(const char* what, hipStream_t s);   // (angular.cpp from here) the first angular call: abundances to HBM, norms
  void norms2(uint64_t* out);
  void angular(ResidentIndex& cols, uint64_t* dot, double* cosine, double* angular);
  void angular_query(const KmerMinHash& query, uint64_t* dot, uint64_t* query_norm2, double* cosine, double* angular);
};

// the loops of find and most_common, shared with their host-sketch forms
inline uint32_t indices_above(const double* val, uint32_t n, double threshold, uint32_t* out_indices) {
  uint32_t k = 0;
  for (uint32_t i = 0; i < n; i++)
    if (val[i] > threshold) out_indices[k++] = i;   // NaN (empty node, containment) is never > threshold
  return k;
}
inline void arg_max(const uint64_t* v, uint32_t n, uint32_t* best_pos, uint64_t* best) {   // null outputs are skipped
  uint32_t pos = 0;
  uint64_t mx = 0;
  for (uint32_t j = 0; j < n; j++)
    if (v[j] > mx) { mx = v[j]; pos = j; }
  if (best_pos) *best_pos = pos;
  if (best) *best = mx;
}

// angular.cpp: the calls that need no index.  rows / cols of angular_block_dev: hashes, abunds and n; offsets on the host
void angular_similarity(const KmerMinHash& a, const KmerMinHash& b, double* angular, double* cosine, uint64_t* dot, uint64_t* norm2_a,
                        uint64_t* norm2_b);
void angular_block_dev(AngularSet rows, const uint64_t* row_offsets, AngularSet cols, const uint64_t* col_offsets,
                       const uint64_t* count_common_dev, bool symmetric, const AngularOut& out, uint64_t* row_norm2_dev,
                       uint64_t* col_norm2_dev, void* stream);
// From g_angular_prune_min_pairs pairs on ResidentIndex::angular first runs the block compare for count_common and walks only the pairs
// that share a hash (default: tools/bench_angular.py's sweep, DESIGN.md 3.10 "The prune threshold").  walked / skipped: of the last call.
constexpr uint64_t kAngularPruneMinPairs = 4096;
extern uint64_t g_angular_prune_min_pairs, g_angular_walked, g_angular_skipped;

// match.cpp: what bounds the work space of match() -- the expected candidates (plus records) of one fold, and the
// (record, node) counters of one round of the tally's dense regime.  The default is a memory cap (about 3.5 GiB of fold
// buffers, 256 MiB of counters), not a measured optimum.
constexpr uint64_t kMatchPairBudget = 1ull << 26;
extern uint64_t g_match_pair_budget;

// match.cpp: the rows of a fold (MatchRow or LcaRow, 24 bytes each) into the caller's array
void fetch_rows(const void* d_rows, void* out, size_t n, Engine& E, hipStream_t s);

// lca.cpp: the taxonomy's refusals alone (kMsg, the message names the entry; index_len: what n_nodes must equal), and the keys
// (query hashes) one chunk of a sketch batch may hold -- a memory cap, not a measured optimum
void lca_check_taxonomy(const uint32_t* parent, uint32_t n_taxa, const uint32_t* node_taxon, uint32_t n_nodes, uint32_t index_len);
constexpr uint64_t kLcaBudget = 1ull << 26;
extern uint64_t g_lca_budget;

// query_batch.cpp: a batch of sketches as one CSR in device memory ("Staging a batch"), for the length of one
// call.  A state that lives in HBM is copied there device to device and is not brought to the host; the host states go up in
// one upload, straight into place when no query lives in HBM.  limit: kQueryLimit32 or kQueryLimit31, what one query may not
// reach.  want_abunds: the abundances behind the hashes when any query tracks them (a query that does not weighs 1 per hash).
// The caller holds the device's lock.  The constructor flushes every query's pending records and returns with the stream
// waited for; its refusals (kInternal, the message begins with `who`) come before anything is allocated.
constexpr uint64_t kQueryLimit32 = 0xffffffffull, kQueryLimit31 = 1ull << 31;
struct QueryBatch {
  QueryBatch(const KmerMinHash* const* queries, uint32_t n_queries, const char* who, uint64_t limit, bool want_abunds, Device& dev);
  const uint64_t* hashes() const { return csr; }
  const uint64_t* abunds() const { return with_abunds ? csr + qoff.back() : nullptr; }   // null: every hash weighs 1
  const uint64_t* offsets() const { return qoff.data(); }   // n_queries + 1, from 0
 private:
  Workspace ws;    // [hashes | abundances], and the host states on their way there when a query lives in HBM
  uint64_t* csr = nullptr;
  std::vector<uint64_t> qoff;
  bool with_abunds = false;
};
// the refusals of a CSR's offsets: "offsets must ascend (query q)" (kMsg), a query of `limit` or more hashes (kInternal)
void check_query_offsets(const char* who, const uint64_t* q_offsets, uint32_t n_queries, uint64_t limit);
// The u32 offsets a chunk's kernels read, those of the queries [a, b) relative to query a (b - a + 1 entries): appended to
// `rel` (returns where they start), or `rel` rewritten with them and uploaded to `dst`.  The upload reads `rel`
// asynchronously: the caller waits for the stream before the next chunk rewrites it (who cannot lays all chunks out first
// and uploads once, as cluster does).
size_t append_chunk_offsets(const uint64_t* q_offsets, uint32_t a, uint32_t b, std::vector<uint32_t>* rel);
void upload_chunk_offsets(const uint64_t* q_offsets, uint32_t a, uint32_t b, std::vector<uint32_t>* rel, uint32_t* dst, hipStream_t s);
// the front half of a search chunk: c zeroed, the probe, the select, and the chunk's row count read back (the stream has been
// waited for when it returns)
uint32_t search_chunk_rows(const MatchDirectory& dir, const SearchChunk& ck, Device& dev, hipStream_t s);

// gather_many.cpp: the (query, node) counters one chunk of a batch may hold (three u32 arrays of that size: 768 MiB at the
// default) -- a memory cap, not a measured optimum.  gather_many_chunk_end: the chunk that starts at query `a` ends in front
// of the returned query -- as many queries as the budget holds counters for, one at least, at most kGatherManyMaxQueries
// (the grid's second dimension) and fewer than 2^32 - 1 positions unless it is a single query.
constexpr uint64_t kGatherManyBudget = 1ull << 26;
constexpr uint32_t kGatherManyMaxQueries = 65535;
extern uint64_t g_gather_many_budget;
// the rule itself (gather_many.cpp), shared with search_many: max_queries is what one grid dimension carries
uint32_t query_chunk_end(const uint64_t* q_offsets, uint32_t a, uint32_t n_queries, uint32_t n_nodes, uint64_t budget, uint32_t max_queries);
uint32_t gather_many_chunk_end(const uint64_t* q_offsets, uint32_t a, uint32_t n_queries, uint32_t n_nodes, uint64_t budget);

// search_many.cpp: the (query, node) counters one chunk of a batch may hold (one u32 array of that size: 256 MiB at the
// default) -- a memory cap, not a measured optimum.  search_many_chunk_end: query_chunk_end with kSearchMaxQueries
// (the grid's second dimension of the select and emit kernels).  check_search: the refusals of a metric
// and a threshold alone (kMsg); needs no device.
constexpr uint64_t kSearchManyBudget = 1ull << 26;
extern uint64_t g_search_many_budget;
uint32_t search_many_chunk_end(const uint64_t* q_offsets, uint32_t a, uint32_t n_queries, uint32_t n_nodes, uint64_t budget);
void check_search(uint32_t metric, double threshold);
// the rows of a search on their way to the caller: malloc'ed (the caller frees them with free()), grown chunk by chunk, one
// element at least; `who` begins the message of the refusal when memory runs out
struct SearchRowsOut {
  const char* who;
  SearchRow* p = nullptr;
  size_t len = 0, cap = 0;
  explicit SearchRowsOut(const char* who_) : who(who_) {}
  SearchRowsOut(const SearchRowsOut&) = delete; SearchRowsOut& operator=(const SearchRowsOut&) = delete;
  ~SearchRowsOut() { free(p); }
  SearchRow* room(size_t more);   // `more` rows behind the ones held
  SearchRow* release() { room(0); SearchRow* r = p; p = nullptr; return r; }
};

// nearest.cpp: the refusal of a k alone (kMsg: 0, or more than kNearestMaxK); needs no device.  The chunks are search_many's,
// under its budget.
void check_nearest_k(uint32_t k);

// cluster.cpp: the directed adjacency entries the greedy linkage may hold in device memory (8 bytes each, 16 while a chunk's
// rows are collected) -- a memory cap, not a measured optimum; the greedy rounds queued between two read-backs of the undecided
// count; check_cluster: the refusals of the arguments alone (kMsg), needs no device.
constexpr uint64_t kClusterPairBudget = 1ull << 27;
extern uint64_t g_cluster_pair_budget;
extern uint32_t g_cluster_rounds;
void check_cluster(uint32_t metric, double threshold, uint32_t linkage, bool want_rep_common);

// collapse.cpp: the refusals of the arguments alone (kMsg; needs no device), and need_g = max(1, min_count, ceil(min_fraction *
// m_g)), the product and the ceiling in IEEE double
void check_collapse(uint32_t n_groups, double min_fraction, uint32_t abund);
uint32_t collapse_need(uint32_t members, uint32_t min_count, double min_fraction);

// index_build.cpp: the expected candidates of one fold of a build (bytes x (max_hash + 1) / 2^64, match's notion).  The default
// is a memory cap -- a candidate takes 32 bytes of sort buffers (40 with their head-room) and a run 20 more, about 4 GiB in
// all -- not a measured optimum; the result never depends on it.  check_index_build: the refusals of the arguments alone
// (kMsg; needs no device), total_len = the bytes the offsets may reach.
enum BuildInput : int { kBuildNucleotide = 0, kBuildAmino = 1 };
constexpr uint64_t kIndexBuildBudget = 1ull << 26;
extern uint64_t g_index_build_budget;
void check_index_build(const KmerMinHash* like, int input, bool have_seq, uint64_t total_len, const uint64_t* offsets, const uint32_t* groups,
                       uint32_t n_records, uint32_t n_groups);
void check_index_concat(ResidentIndex* const* parts, uint32_t n_parts);

// filter.cpp: every refusal of a filter that needs no device (kMsg, the message begins with "filter:"; an operand that is
// incompatible with the nodes: 101-104 from check_sketch).  check_filter_rule: those of the rule alone (a null rule, an unknown
// mode, min > max, OPERAND without KEEP_IN), for callers that have no index yet; check_filter runs it first.
void check_filter_rule(const FilterRule* rule);
void check_filter(const ResidentIndex& index, const KmerMinHash* operand, const FilterRule* rule);
void check_index_select(const ResidentIndex& index, const uint32_t* ids, uint32_t n_ids);

// downsample.cpp (the rules are in include/sourmash_amd.h, "Downsampling").  `out` is a fresh sketch: it
// receives src's parameters with max_hash / num replaced and the kept prefix.  A state that lives in HBM is cut there into a
// DeviceSketch of out's own; neither sketch is brought to the host.
void downsample_max_hash(const KmerMinHash& src, uint64_t max_hash, KmerMinHash& out);
void downsample_num(const KmerMinHash& src, uint32_t num, KmerMinHash& out);   // host only
// the bounds pass of a CSR and its read-back (4 bytes per sketch): new_off = the n + 1 offsets of the kept prefixes, from 0;
// returns the longest of them
uint32_t downsample_bounds_host(const uint64_t* hashes_dev, const uint64_t* offsets_dev, uint32_t n, uint64_t max_hash,
                                std::vector<uint64_t>* new_off, Device& dev, hipStream_t s);
// a CSR in device memory (offsets on the host, n + 1) cut into caller's buffers; out_offsets (host, n + 1) start at 0
void downsample_block_dev(const uint64_t* hashes_dev, const uint32_t* abunds_dev, const uint64_t* offsets, uint32_t n, uint64_t max_hash,
                          uint64_t* out_hashes_dev, uint32_t* out_abunds_dev, uint64_t capacity, uint64_t* out_offsets, void* stream);

}  // namespace smh
