// kernels.hpp -- launch interfaces of the HIP kernels (sketch_kernels.hip and sketch_{dna,protein,amino}_kernels.hip, sort.hip,
// compare_kernels.hip, parse_kernels.hip, gather_kernels.hip, angular_kernels.hip, downsample_kernels.hip, match_kernels.hip,
// gather_many_kernels.hip, lca_kernels.hip, search_many_kernels.hip, cluster_kernels.hip, collapse_kernels.hip,
// index_build_kernels.hip, filter_kernels.hip, nearest_kernels.hip, inflate_kernels.hip, archive_kernels.hip).
// Plain structs and pointers; no torch types anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "device.hpp"

namespace smh {

// Where the hash kernels append the hashes that pass the threshold.  `count` keeps counting
// past `capacity`, so an overflowing launch reports exactly how much room a re-run needs.
struct CandSink {
  uint64_t* hash = nullptr;
  uint64_t* pos = nullptr;  // stream position of the k-mer (only when order matters: Q3/Q4)
  unsigned long long* count = nullptr;
  uint64_t capacity = 0;
};

// One flat byte buffer holding 1..nrec records.  Record r is [starts[r], starts[r+1]);
// bytes at or beyond vends[r] are not part of it (force=false truncation, reference
// src/lib.rs:268-273).  starts == nullptr means a single record [0, len) ending at vend0.
struct SeqBatch {
  const uint8_t* seq = nullptr;
  uint64_t len = 0;
  const uint64_t* starts = nullptr;
  const uint64_t* vends = nullptr;
  uint32_t nrec = 1;
  uint64_t vend0 = 0;
  // set by the launchers of the tiled kernels: per tile of the launch, the record that holds its first
  // position (see k_tile_records)
  const struct TileRec* tile_rec = nullptr;
};

struct TileRec {
  uint32_t rec;    // record of the tile's first position
  uint32_t last;   // record of the first position of the NEXT tile (== rec: the tile lies inside one record)
  uint64_t end;    // end of the valid part of `rec`
};

struct HashParams {
  uint32_t ksize = 31;
  uint32_t alphabet = 0;              // protein arm and amino-acid input: the sketch's Molecule (0 / 1: residues as they are)
  uint64_t seed = 42;
  const uint64_t* thr_rec = nullptr;  // DNA arm: per-record thresholds (device, nrec entries) or null
  uint64_t thr = ~0ull;               // the threshold when thr_rec is null (and the LDS stage estimate)
  uint64_t pos_base = 0;
  uint64_t range_lo = 0, range_hi = 0;  // k-mer start positions [lo, hi) handled by this launch
};

// --- sketch_dna_kernels.hip: launch_dna_hash, launch_first_invalid, launch_first_bad_record, launch_record_stats;
// --- sketch_protein_kernels.hip: launch_translate, launch_protein_fused, launch_hash_windows;
// --- sketch_amino_kernels.hip: launch_amino_hash, amino_geometry; the others: sketch_kernels.hip ---
// DNA arm of add_sequence (reference src/lib.rs:258-274): canonical k-mer + murmur64 + filter.
// Picks the rolling 2-bit kernel for ksize <= 32 and the byte-wise kernel otherwise.
void launch_dna_hash(const SeqBatch& b, const HashParams& p, const CandSink& sink, Device& dev,
                     hipStream_t s, bool force_generic = false);

// smallest position of a byte outside [ACGTacgt] per record -> vends (atomicMin); vends must be
// pre-filled with the record ends.  (reference src/lib.rs:795-804 _checkdna, applied per byte)
void launch_first_invalid(const SeqBatch& b, uint64_t* vends_out, hipStream_t s);
// *out (device) = the first record that is at least ksize long and whose vends entry lies before its end, else UINT64_MAX
void launch_first_bad_record(const uint64_t* starts, const uint64_t* vends, uint32_t nrec, uint32_t ksize, uint64_t* out, hipStream_t s);
// out2 (device): [0] records of at least ksize bases, [1] positions of the protein arm's six-frame layout
void launch_record_stats(const uint64_t* starts, uint32_t nrec, uint32_t ksize, uint64_t* out2, hipStream_t s);

// launch_hash_segments: murmur64 of whole byte strings (add_word / hash_murmur, reference
// src/lib.rs:247-250, src/ffi.rs:15-24) -> out[i].
// launch_hash_windows: every window of `win` kept residues inside each segment of the translated
// buffer (protein arm second phase, reference src/lib.rs:289-300) -> candidate sink.
void launch_hash_segments(const uint8_t* bytes, const uint64_t* seg_offsets, uint32_t nseg,
                          uint64_t seed, uint64_t* out, hipStream_t s);
void launch_hash_windows(const uint8_t* bytes, uint64_t total, const uint64_t* seg_offsets,
                         uint32_t nseg, uint32_t win, const HashParams& p, const CandSink& sink,
                         hipStream_t s);

// six-frame translation (reference src/lib.rs:277-301, 779-793).  seg_offsets (device, nseg+1
// entries, nseg = 6*nrec) gives where each (record, frame, strand) segment lives in `residues`;
// unknown codons are written as 0xFF and skipped by launch_hash_windows; bad_utf8[seg] is set when
// a codon chunk is not valid UTF-8 (the reference panics there).
void launch_translate(const SeqBatch& b, const uint64_t* seg_offsets, uint32_t nseg, uint64_t total, uint32_t ksize, uint32_t alphabet,
                      uint8_t* residues, uint32_t* bad_utf8, hipStream_t s);

// Protein arm in ONE pass over the DNA (translation + hashing, no residue buffer): every window of
// `win` residues of the six frames of the whole batch (p.range_* are not used); candidate positions,
// when the sink wants them, are indices of the six-frame layout (seg_offsets, as above) + p.pos_base.
// b.vend0 (single record) must be 0
// when the record is shorter than p.ksize.  *high_flag is OR-ed with 1 when the batch holds a byte
// >= 0x80: the result must then be discarded and the two-pass path taken (UTF-8 panic semantics).
// Returns false (nothing launched) for window lengths it has no instantiation for.
bool launch_protein_fused(const SeqBatch& b, const uint64_t* seg_offsets, uint32_t win, const HashParams& p,
                          const CandSink& sink, uint32_t* high_flag, Device& dev, hipStream_t s);

// Amino-acid input: every window of `win` bytes that lies inside one record and starts in [p.range_lo, p.range_hi), each
// byte upper-cased and mapped through p.alphabet; a candidate's position is p.pos_base + the byte offset of its window
// start.  win <= 64: k_amino_tiled (profile name amino_tiled), else k_amino_generic (amino_generic).  b.vends is not used.
void launch_amino_hash(const SeqBatch& b, uint32_t win, const HashParams& p, const CandSink& sink, Device& dev, hipStream_t s);
// window starts per workgroup tile and per lane of such a launch (one geometry; 256 / 1 for the generic kernel)
void amino_geometry(uint64_t total_len, uint32_t win, uint32_t* tile_positions, uint32_t* run);

// hashes[lo..hi) that are <= thr go to the sink with their index as stream position
// (bulk add_many, reference src/lib.rs:412-417)
void launch_filter_hashes(const uint64_t* hashes, const HashParams& p, const CandSink& sink, hipStream_t s);

// synthetic DNA generator (same definition as oracle osynth_dna)
void launch_synth_dna(uint8_t* out, uint64_t start, uint64_t len, uint64_t seed, uint64_t n_every,
                      hipStream_t s);

// --- parse_kernels.hip -----------------------------------------------------------------
// FASTA / FASTQ text in device memory -> dense sequence bytes + record offsets + name spans.
enum ParseFormat : int { kFormatAuto = 0, kFormatFasta = 1, kFormatFastq = 2 };
constexpr uint32_t kParseTileBytes = 4096;   // tiles are cut on 16-byte boundaries of the address: the first may hold fewer text bytes
// The state a tile is entered in.  The first tile's is the caller's: a text parsed in one go starts with all zero.
struct ParseTileIn {
  uint64_t outpos;   // kept bytes in front of the tile
  uint64_t count;    // FASTA: records started in front of it; FASTQ: '\n' bytes in front of it (= the running line's number)
  int64_t bal;       // FASTQ: sequence bytes - quality bytes in front of it
  uint32_t cls;      // FASTA: class of the running line (0 none, 1 sequence, 2 header)
  uint32_t pad;
};
struct ParseTotals {
  uint64_t n_records, total, lines;   // lines: FASTQ, after the empty ones at the end are dropped
  int64_t balance;
  uint64_t err;                       // ~0: none; FASTA: byte offset of data in front of the first header; FASTQ: lowest malformed record
};
size_t parse_workspace_bytes(const void* text, uint64_t len);
// *out_dev = the first byte of the text that belongs to no line terminator (~0: there is none)
void launch_first_content(const uint8_t* text, uint64_t len, uint64_t* out_dev, hipStream_t s);
// passes 1 and 2: tile summaries and their scan into `workspace`; *totals_dev is written (err included)
void launch_parse_scan(int format, const uint8_t* text, uint64_t len, const ParseTileIn& first, void* workspace,
                       ParseTotals* totals_dev, hipStream_t s);
// pass 3, with the totals read back: out (16-byte aligned, totals.total bytes), offsets / name_start / name_end
// (totals.n_records entries each); totals_dev->err is lowered by the format checks
void launch_parse_compact(int format, const uint8_t* text, uint64_t len, const void* workspace, const ParseTotals& totals,
                          uint8_t* out, uint64_t* offsets_dev, uint64_t* name_start_dev, uint64_t* name_end_dev,
                          ParseTotals* totals_dev, hipStream_t s);
// records.cpp.  The records of one text: the compacted sequence bytes and the name spans in HBM, the offsets on the host
// (page-locked: the sketching paths walk them and upload them again).  Holds no reference to the text.
struct Records {
  std::unique_ptr<PoolBlock> seq, names;            // total + 64 bytes; name_start[n], name_end[n] (they wait for the device when freed)
  uint64_t* offsets = nullptr;                      // n + 1, hipHostMalloc
  uint32_t n = 0;
  uint64_t total = 0;
  int format = 0;
  ~Records() { if (offsets) (void)hipHostFree(offsets); }
  const uint8_t* seq_dev() const { return seq ? seq->as<uint8_t>() : nullptr; }
  void name_spans(uint64_t* start_out, uint32_t* len_out) const;   // n entries each, read back from `names`
};
// fills a new *rec from a text in device memory (on the caller's `stream`) or in host memory (uploaded first, own stream)
void parse_records(Records* rec, const void* text, bool text_on_host, uint64_t len, int format, void* stream, Device& dev);

// --- inflate_kernels.hip, inflate.cpp --------------------------------------------------
// Blocked gzip (BGZF) inflated on the device (the rules are in include/sourmash_amd.h, "Blocked gzip").
constexpr uint32_t kInflateThreads = 256;    // four waves per workgroup, one member per wave and trip
struct InflateMember {                       // one gzip member of the chain, as the host scan found it
  uint64_t payload_off;                      // the DEFLATE stream: data[payload_off, payload_off + payload_len)
  uint64_t out_off;                          // its text: out[out_off, out_off + isize)
  uint32_t payload_len, isize, crc, pad;
};
// status[m] = the inflate::Reason of member m; *err (caller: all ones) is lowered to (m << 8 | reason) by every bad member.
// Profile name inflate.
void launch_inflate(const uint8_t* data, const InflateMember* members, uint64_t n_members, uint8_t* out, bool verify_crc, uint8_t* status,
                    unsigned long long* err, Device& dev, hipStream_t s);
// The member table of one chain (host only: no device is touched).
struct Gzip {
  std::vector<InflateMember> members;
  std::vector<uint64_t> header_off;          // where each member starts in the file (error messages)
  uint64_t len = 0, inflated = 0;            // bytes scanned; sum of the ISIZEs
};
void gzip_scan(Gzip* g, const uint8_t* data, uint64_t len);   // throws Error(kMsg)
// data_dev: the len scanned bytes in device memory.  status_out: host, one byte per member, or null.  Returns with the work
// complete; throws Error(kMsg) naming the lowest bad member (status_out is filled first).
void gzip_inflate_dev(const Gzip& g, const uint8_t* data_dev, uint64_t len, uint8_t* out_dev, uint64_t out_cap, bool verify_crc,
                      uint8_t* status_out, hipStream_t s, Device& dev);
void gzip_inflate_host(const uint8_t* data, uint64_t len, uint8_t* out_dev, uint64_t out_cap, bool verify_crc, uint8_t* status_out,
                       Device& dev);

const char* inflate_reason_text(uint32_t reason);   // the words of an inflate::Reason (error messages)

// --- archive_kernels.hip, archive.cpp --------------------------------------------------
// Zip collections inflated on the device (the rules are in include/sourmash_amd.h, "Zip collections").
struct ArchiveMember {                       // one id of a call: what is read, where its text goes
  uint64_t src_off;                          // the DEFLATE stream, or a stored entry's bytes: data[src_off, src_off + src_len)
  uint64_t out_off;                          // its text: out[out_off, out_off + size)
  uint32_t src_len, size, crc, inflated;     // crc: the text's expected CRC-32; inflated: 1 DEFLATE, 0 stored (a copy)
};
// status[m] = the inflate::Reason of order[...] = m; *ticket is zero; *err as launch_inflate's.  Profile name archive_inflate.
void launch_inflate_queue(const uint8_t* data, const ArchiveMember* members, const uint64_t* order, uint64_t n_order, unsigned long long* ticket,
                          uint8_t* out, uint8_t* status, unsigned long long* err, Device& dev, hipStream_t s);
// prefix: n_members + 1 chunk counts summed (archive_core.hpp); terms: one register per chunk.  Copies the stored members;
// verify: also leaves every chunk's CRC register.  Profile name archive_chunks.
void launch_archive_chunks(const uint8_t* data, const ArchiveMember* members, const uint64_t* prefix, uint64_t n_members, uint64_t n_chunks,
                           uint8_t* out, uint32_t* terms, bool verify, Device& dev, hipStream_t s);
// folds the registers of every member whose status is still ok and compares.  Profile name archive_crc.
void launch_archive_crc(const ArchiveMember* members, const uint64_t* prefix, uint64_t n_members, const uint32_t* terms, uint8_t* status,
                        unsigned long long* err, Device& dev, hipStream_t s);
namespace archive { struct Archive; }
void archive_scan(archive::Archive* a, const uint8_t* data, uint64_t len);   // host only; throws Error(kMsg)
// ids: n_ids entries of the scan, any order, repeats allowed; entry ids[i] becomes out[out_offs[i], + its text size).
// status_out: host, one byte per id, or null.  Returns with the work complete; throws Error(kMsg) naming the entry of the
// lowest bad position (status_out is filled first).
void archive_inflate_dev(const archive::Archive& a, const uint8_t* data_dev, uint64_t len, const uint32_t* ids, const uint64_t* out_offs,
                         uint64_t n_ids, uint8_t* out_dev, uint64_t out_cap, bool verify, uint8_t* status_out, hipStream_t s, Device& dev);
void archive_inflate_host(const archive::Archive& a, const uint8_t* data, uint64_t len, const uint32_t* ids, const uint64_t* out_offs,
                          uint64_t n_ids, uint8_t* out_dev, uint64_t out_cap, bool verify, uint8_t* status_out, Device& dev);
extern bool g_archive_sorted;   // a measurement knob (smh_archive_set_sorted; default true): false hands members out in id order

// --- sigscan_kernels.hip ---------------------------------------------------------------
// Signature JSON text in device memory -> the u64 values of its number arrays, one row per span, and the skeleton
// (the rules are in include/sourmash_amd.h, "Signature JSON on the device", the automaton in sigscan_core.hpp).
constexpr uint32_t kSigThreads = 256;
constexpr uint32_t kSigTileBytes = 4096;   // tiles are cut on 16-byte boundaries of the address, as the parser's are
struct SigTotals {
  uint64_t skeleton, spans, tokens;        // bytes kept, spans opened, tokens started
  uint32_t final_state, pad;               // the sigscan::State the text ends in
};
struct SigSpanDev {                        // one span as the compaction leaves it; the caller fills the rows with all ones first
  uint64_t start, end, first_token, end_token;   // end stays all ones for a span that runs to the end of the text
  uint64_t bad_syntax, overflow;                 // the lowest offending byte of either kind, all ones: none
  uint32_t last_state, pad;
};
void sigscan_geometry(uint32_t* tile_bytes, uint32_t* threads);
size_t sigscan_workspace_bytes(const void* text, uint64_t len);
// passes 1 and 2 (profile names sigscan_summary, sigscan_scan): tile summaries and their scan into `workspace`; *totals_dev is written
void launch_sigscan_scan(const uint8_t* text, uint64_t len, void* workspace, SigTotals* totals_dev, Device& dev, hipStream_t s);
// pass 3 (sigscan_compact), with the totals read back: skeleton (totals.skeleton bytes), rows (totals.spans), values (totals.tokens)
void launch_sigscan_compact(const uint8_t* text, uint64_t len, const void* workspace, const SigTotals& totals, uint8_t* skeleton,
                            SigSpanDev* rows, uint64_t* values, Device& dev, hipStream_t s);
// The checks of a CSR gathered from the values (hashes, offsets_dev: n + 1 from 0, total = offsets[n]): *err (caller: all ones) is
// lowered to node << 32 | position by every hash not above its predecessor in the node.  out_abunds non-null: node v's abundances are
// values[abund_src_dev[v] ..), narrowed to 32 bits (2^32 or more: all ones, counted in *n_wide, its place appended to wide_pos when
// that is given and holds fewer than wide_cap).
void launch_sigscan_gather_check(const uint64_t* hashes, const uint64_t* offsets_dev, uint32_t n, uint64_t total, const uint64_t* values,
                                 const uint64_t* abund_src_dev, uint32_t* out_abunds, unsigned long long* err, unsigned long long* n_wide,
                                 uint64_t* wide_pos, uint64_t wide_cap, Device& dev, hipStream_t s);

// --- sigtext_kernels.hip ---------------------------------------------------------------
// A resident index -> the decimal text of its arrays and every node's md5 (the rules are in
// include/sourmash_amd.h, "Signature JSON written on the device", the shared pieces in sigtext_core.hpp).
constexpr uint32_t kSigTextThreads = 256;
constexpr uint32_t kSigTextTile = 1024;     // values per workgroup trip of the measure and emit passes (four per thread)
constexpr uint32_t kSigTextMd5Step = 64;    // values a wave formats between two runs of the block function
inline uint64_t sigtext_tiles(uint64_t total) { return (total + kSigTextTile - 1) / kSigTextTile; }
struct SigTextPass {                        // the CSR as the kernels read it: values counted from off[0]
  const uint64_t* hashes = nullptr;         // total of them (the pointer stands at element off[0])
  const uint32_t* abunds = nullptr;         // likewise; null: an index without abundances (tile_a, node_a are then not touched)
  uint64_t total = 0;
  const uint64_t* off = nullptr;            // n + 1 node boundaries, device
  uint32_t n = 0;
  uint64_t *tile_h = nullptr, *tile_a = nullptr;   // sigtext_tiles(total) + 1 each: digit sums per tile, scanned in place (exclusive)
  uint64_t *node_h = nullptr, *node_a = nullptr;   // n + 1 each: the digit prefix at every node boundary
};
struct SigTextPlace {                       // where everything goes, as the host laid it out
  const uint8_t* skeleton = nullptr;        // the pieces one after another
  uint64_t skeleton_len = 0;
  const uint64_t *piece_src = nullptr, *piece_dst = nullptr;   // pieces + 1 starts in the skeleton; pieces places in the text
  uint64_t pieces = 0;
  const uint64_t *mins_at = nullptr, *abunds_at = nullptr;     // n each: where the inside of a node's array begins
  const uint8_t* digests = nullptr;         // 16 n bytes, launch_sigtext_md5's
  const uint64_t* md5_at = nullptr;         // n: where a node's 32 hex digits stand
  uint8_t* text = nullptr;
  uint64_t text_len = 0;
};
void sigtext_geometry(uint32_t* values_per_tile, uint32_t* threads, uint32_t* md5_values_per_step);
// passes 1 and 2 (profile names sigtext_measure, sigtext_scan): tile_*, node_* are written
void launch_sigtext_measure(const SigTextPass& p, Device& dev, hipStream_t s);
// pass 3 (sigtext_emit): the skeleton pieces, both arrays of every node and, over the placeholders, the digests as lower-case hex
void launch_sigtext_emit(const SigTextPass& p, const SigTextPlace& w, Device& dev, hipStream_t s);
// pass 4 (sigtext_md5): digests[16 v ..) = the md5 of str(ksizes[v]) and node v's decimal hashes; hashes stands at element off[0]
void launch_sigtext_md5(const uint64_t* hashes, const uint64_t* off, uint32_t n, const uint32_t* ksizes, uint8_t* digests, Device& dev,
                        hipStream_t s);

// --- sort.hip -----------------------------------------------------------------------
// LSD radix sort, ping-pong between (k0,v0) and (k1,v1); returns which pair holds the result.
// Only the byte passes [first_pass, last_pass) are run (default: all eight): a stable sort by a bit
// field of the key.
int radix_sort_u64(uint64_t* k0, uint64_t* k1, uint64_t* v0, uint64_t* v1, size_t n,
                   DeviceBuffer& scratch, hipStream_t s, int first_pass = 0, int last_pass = 8, uint32_t pass_mask = 0);
// The whole fold of a small batch in ONE launch that reads the candidate count from device memory (no host round trip in
// front of it): up to kSmallFoldMax candidates -> distinct keys ascending in uniq, their run starts in starts (both with room
// for kSmallFoldMax entries), result_dev[0] = candidates, result_dev[1] = runs.  More candidates than it takes (kSmallFoldMax,
// or half of that when `expected` is small enough for the half-size instance), or than `capacity`: result_dev[1] = ~0 and
// nothing else is written.
constexpr uint32_t kSmallFoldMax = 16384;
void small_fold_async(const uint64_t* keys, const unsigned long long* count_dev, uint64_t capacity, uint64_t* uniq, uint32_t* starts,
                      unsigned long long* result_dev, uint32_t expected, hipStream_t s);
// the same with a 32-bit payload (indices): a quarter less traffic per pass
// pass_mask != 0: run exactly the byte passes whose bit is set instead of reading the digit histograms
// back to skip constant bytes -- no host synchronisation inside the sort
int radix_sort_u64_v32(uint64_t* k0, uint64_t* k1, uint32_t* v0, uint32_t* v1, size_t n, DeviceBuffer& scratch,
                       hipStream_t s, uint32_t pass_mask = 0);
int radix_sort_u64_keys(uint64_t* k0, uint64_t* k1, size_t n, DeviceBuffer& scratch, hipStream_t s, uint32_t pass_mask);
// keys[0 .. n) (read only) sorted into k0 or k1 (the return value says which), v0 / v1 alongside = where every sorted key
// was in `keys`: the first pass reads `keys` and numbers them itself -- no copy of the keys, no index array.  pass_mask != 0.
// shift_dev (nullable): a device word added to every pass's shift -- pass p sorts by bits [*shift_dev + 8 p, + 8): the caller's
// passes start at a bit only the device knows (the low end of the 32 most significant bits that vary, see k_key_span).
int radix_sort_u64_place(const uint64_t* keys, uint64_t* k0, uint64_t* k1, uint32_t* v0, uint32_t* v1, size_t n, DeviceBuffer& scratch,
                         hipStream_t s, uint32_t pass_mask, const uint32_t* shift_dev = nullptr);
// run_length_encode_u64 without its read-back: *nruns_dev (device) receives the number of runs;
// skip (device, nullable): non-zero = the launches do nothing
void run_length_encode_u64_async(const uint64_t* keys, size_t n, uint64_t* uniq, uint32_t* starts, DeviceBuffer& scratch,
                                 hipStream_t s, const uint32_t* origin, uint32_t* rank_out, uint32_t* nruns_dev,
                                 const uint32_t* skip, uint32_t* runid_out = nullptr,    // runid_out[i] = run of sorted position i
                                 bool rank_flags = false);   // rank_out values carry bit 31 = run longer than 1, bit 30 = first of its run
// in-place exclusive scan of m u32 counters; *total (device, nullable) receives their sum
void exclusive_scan_u32_dev(uint32_t* d, size_t m, uint32_t* total, DeviceBuffer& scratch, hipStream_t s);
// unique keys + run start indices of a sorted array; returns the number of runs (syncs).
// origin / rank_out (optional): also write rank_out[origin[i]] = run id of sorted position i.
// key2 / uniq2 (optional): a more significant second key (array sorted by (key2, keys)); a run
// ends where either changes and uniq2[run] receives its key2.
uint32_t run_length_encode_u64(const uint64_t* keys, size_t n, uint64_t* uniq, uint32_t* starts,
                               DeviceBuffer& scratch, hipStream_t s, const uint32_t* origin = nullptr,
                               uint32_t* rank_out = nullptr, const uint64_t* key2 = nullptr,
                               uint64_t* uniq2 = nullptr, int key2_shift = 0);   // key2 is compared as key2 >> key2_shift
// Union of a device-resident sketch S (ascending distinct hashes + optional u64 counts, which are UPDATED in place for the
// hashes D also holds) with the fold D of one more batch (ascending distinct hashes + optional run starts): out / out_cnt
// (room for n_s + n_d entries) receive the merged sketch, *n_new_dev the number of hashes that were new (result size =
// n_s + that).  tmp: (2 n_d + n_s + 1) u32 of work space.  No sort, no host round trip.
void sorted_union_async(const uint64_t* S, uint64_t* S_cnt, uint32_t n_s, const uint64_t* D, const uint32_t* D_starts,
                        const uint64_t* D_cnt /* counts of D: these, or run starts, when S_cnt is given */, uint32_t n_d, uint32_t d_total, uint64_t* out, uint64_t* out_cnt, uint32_t* n_new_dev, DeviceBuffer& tmp, DeviceBuffer& scratch,
                        hipStream_t s);
// counts[i] = starts[i+1] - starts[i] (the last run ends at total)
void starts_to_counts(const uint32_t* starts, uint32_t n, uint32_t total, uint64_t* counts, hipStream_t s);
// cand_pos[i] (a k-mer start position of the batch) -> the sketch group of the record holding it
// keep_bits != 0: the position is kept in the low keep_bits bits, the group goes above them
void launch_pos_to_group(uint64_t* pos, uint64_t n, const uint64_t* rec_starts, uint32_t nrec,
                         const uint32_t* group_of_rec, hipStream_t s, int keep_bits = 0);
// reduces the first `nruns` of `total_runs` runs (run u ends at starts[u+1], the last one at n)
void run_reduce(const uint32_t* starts, uint32_t nruns, uint32_t total_runs, uint32_t n,
                const uint64_t* weights, const uint64_t* pos, uint64_t* out_sum, uint64_t* out_minpos,
                hipStream_t s);

// --- compare_kernels.hip ---------------------------------------------------------------
// Sketches as CSR: hashes[offsets[i] .. offsets[i+1]) ascending and unique.
struct SketchSet {
  const uint64_t* hashes = nullptr;
  const uint64_t* offsets = nullptr;  // n+1 entries (device)
  uint32_t n = 0;
  const uint64_t* h_offsets = nullptr;  // the same n+1 entries in host memory when the caller has them (saves a read-back)
};
struct CompareOut {
  uint64_t* common = nullptr;  // |A ^ B ^ bottom_n(A u B)|   (reference src/lib.rs:470-499)
  uint64_t* size = nullptr;    // |bottom_n(A u B)|
  double* jaccard = nullptr;   // common / max(1, size)        (reference src/lib.rs:501-508)
  uint64_t* count_common = nullptr;  // |A ^ B| untruncated     (reference src/lib.rs:428-436)
  double* containment = nullptr;     // |A ^ B| / |A|           (reference src/index.rs:146-154)
};
// The outputs of an np-pair block for a caller that wants them on the host: five device slots of np entries carved from
// `buf` (room for tail_bytes more behind them, at tail()); dev_out() points only at the slots whose host pointer is set --
// without count_common / containment the kernels may stop at the cut -- and fetch() queues those slots' copies back.
struct HostCompareOut {
  void* host[5];   // in CompareOut's order
  uint64_t* dev;
  size_t np;
  HostCompareOut(DeviceBuffer& buf, size_t np_, uint64_t* common, uint64_t* size, double* jaccard, uint64_t* count_common,
                 double* containment, size_t tail_bytes = 0) : host{common, size, jaccard, count_common, containment}, np(np_) {
    buf.ensure(np * 8 * 5 + tail_bytes + 64);
    dev = buf.as<uint64_t>();
  }
  template <class T> T* slot(int k) const { return host[k] ? reinterpret_cast<T*>(dev + k * np) : nullptr; }
  CompareOut dev_out() const { return {slot<uint64_t>(0), slot<uint64_t>(1), slot<double>(2), slot<uint64_t>(3), slot<double>(4)}; }
  void* tail() const { return dev + 5 * np; }
  void fetch(hipStream_t s) const {
    for (int k = 0; k < 5; k++) if (host[k]) HIP_CHECK(hipMemcpyAsync(host[k], dev + k * np, np * 8, hipMemcpyDeviceToHost, s));
  }
};
// rows x cols block; num = truncation length of the union walk (row's `num`; 0 = unbounded),
// row_nums (device, nullable) overrides it per row.
// max_row_len / max_col_len: longest sketch on each side (decides LDS staging).
// one ordered pair from plain device pointers; out = {|A u B|, |A n B|, common within the first n of the union}
struct PairOut { unsigned long long tot_u, tot_c, common; };
void launch_compare_pair(const uint64_t* A, uint32_t la, const uint64_t* B, uint32_t lb, uint64_t n, PairOut* out_dev,
                         Device& dev, hipStream_t s);

// Which kernel serves an N x M block is chosen from its shape.  The choice never changes a result;
// it can be pinned (parity tests force every route over the same inputs, callers may know better).
enum CompareRoute : uint32_t { kRouteAuto = 0, kRouteWave = 1, kRouteFew = 2, kRouteComponents = 3, kRouteTiled = 4 };
struct CompareTuning {
  uint32_t route = kRouteAuto;             // kRouteComponents / kRouteTiled both mean "the block path"; the two
                                           // are told apart by comp_pairs_limit
  uint32_t visit_all_tiles = 0;            // 1: launch every tile, not only those that can hold sharing pairs
  uint32_t use_symmetry = 1;               // all-vs-all with one num: compute the upper triangle, mirror the rest
  uint32_t split_frequent = 1;             // hashes held by a large share of the sketches do not make components
  uint32_t dictionary = 0;                 // 1: the pooled sort of the dictionary with all eight byte passes (default: four + tie fix)
  uint32_t no_range_masks = 0;             // 1: the tiled kernel walks every pair from the first range on (default: range masks)
  uint64_t comp_pairs_limit = 96ull << 10;  // at most this many sharing pairs: per-component pair kernel, else tiled (the pair kernel
                                           // takes ~3.7 ns per pair of num = 2000 sketches, one round of tiles ~0.45 ms: profiles/r03_tile_shape.txt)
};
struct CompareStats {                      // of the last block compare
  uint32_t route = 0;                      // CompareRoute that ran
  uint32_t rows_per_tile = 0;
  uint64_t tiles_visited = 0, tiles_total = 0, pairs_per_tile = 0;   // components route: pairs walked / pairs / 1
  uint64_t lds_overflow_steps = 0;         // tiled: (tile, range) steps merged from global memory instead of LDS
  uint32_t frequent_hashes = 0;            // hashes set aside as frequent (decided from per-sketch positions, not walked)
  uint32_t pipelined = 0;                  // tiled: k_compare_tiled_pf walked the tiles
  uint32_t span_halvings = 0;              // pipelined kernel: stretches rebuilt with a halved span (their speculative span did not fit LDS)
  uint32_t prefetched_after_halving = 0;   // ... tiles in which prefetched crossings were used after such a rebuild
  uint32_t range_masks = 0;                // tiled: the kernel read the range masks (not in SmhCompareStats: smh_compare_last_range_masks)
};
void compare_set_tuning(const CompareTuning& t);
CompareTuning compare_get_tuning();
CompareStats compare_last_stats();
void release_compare_scratch();   // frees the tiled kernel's pre-pass buffers
// The dictionary of one collection of sketches resident in HBM (CSR; element t of the collection is hashes_dev[offsets[0] + t]):
// dense ranks of all its hashes, components, frequent hashes, range tables -- built once, by one owner or by `world`
// cooperating owners (each holding the same CSR; owner `rank` sorts slice `rank` of hash space) with ONE all-gather of
// collection_share() between collection_begin and collection_finish; then any number of block compares over it.
// own_mode of collection_compare: 0 every pair of the block; 1 rows == columns == the whole collection with one num
// (upper triangle + mirrors); 2 the rows are one rank's block of the all-vs-all matrix, columns == everything, one num:
// only pairs (i, j) with (j - i) mod N < N/2 (ties: i < j) must be computed here, the others arrive from their owner's rank.
struct CollectionDict;
CollectionDict* collection_begin(const uint64_t* hashes_dev, const uint64_t* offsets_dev /*nullable*/, const uint64_t* offsets_host,
                                 uint32_t n, uint32_t world, uint32_t rank, Device& dev, hipStream_t s);
uint64_t collection_share_bytes(const CollectionDict* d);
const void* collection_share(const CollectionDict* d);
uint32_t collection_len(const CollectionDict* d);
void collection_finish(CollectionDict* d, const void* gathered_dev, Device& dev, hipStream_t s);
void collection_compare(CollectionDict* d, uint32_t row_lo, uint32_t row_hi, uint32_t col_lo, uint32_t col_hi, uint32_t num,
                        const uint32_t* row_nums, uint32_t own_mode, const CompareOut& out, Device& dev, hipStream_t s);
void collection_free(CollectionDict* d);

// the mirrored-block exchange of a matrix computed with own_mode 2 (8-byte elements): the block this rank sends to the rank
// holding rows [col_lo, col_hi) -- its own block's columns, transposed -- and what it keeps of a block it received
void launch_mirror_pack(const void* out, uint32_t n_local, uint32_t n_total, uint32_t col_lo, uint32_t col_hi, void* packed, hipStream_t s);
void launch_mirror_apply(void* out, uint32_t row_lo, uint32_t n_local, uint32_t n_total, uint32_t peer_lo, uint32_t peer_hi, const void* recv,
                         hipStream_t s);

void launch_compare_block(const SketchSet& rows, const SketchSet& cols, uint32_t num,
                          const uint32_t* row_nums, const CompareOut& out, Device& dev,
                          hipStream_t s, uint32_t max_row_len, uint32_t max_col_len, uint64_t nr_elems,
                          uint64_t nc_elems, bool same_sets = false);   // same_sets: rows and cols are one CSR

// --- gather_kernels.hip ----------------------------------------------------------------
// Gather: the greedy decomposition of one scaled query against a resident set.  In round r the sketch with
// the largest count of still unassigned query positions wins (lowest index on ties), is reported as row r and its positions
// are labelled r; it ends when the best count is below `threshold` (0 is read as 1) or `capacity` rows are written.
struct GatherRow {
  uint32_t match;              // index of the winning sketch
  uint32_t common_remaining;   // |A_r ^ S_match|: query positions it consumed
  uint32_t common_original;    // |Q ^ S_match|
  uint32_t size_match;         // |S_match|
  uint64_t abund_sum;          // sum of the query's abundances over the consumed positions
};
struct GatherQuery {           // ascending distinct hashes in device memory; abundances: u64 counts, or run starts, or none (1 each)
  const uint64_t* hashes = nullptr;
  uint32_t n = 0;
  const uint64_t* counts = nullptr;
  const uint32_t* starts = nullptr;   // abundance p = starts[p + 1] - starts[p], the last run ends at total
  uint32_t total = 0;
};
constexpr uint32_t kGatherRoundsPerSync = 32;   // rounds queued between two 8-byte read-backs of {done, rounds}
// idx needs h_offsets.  rows_host: room for min(capacity, idx.n) rows; assigned_host (nullable): q.n entries, the round that
// consumed each query position or 0xffffffff.  Returns the number of rows; the stream is idle when it returns, and every
// block it took from the device pool is back there.
uint32_t gather_run(const SketchSet& idx, uint32_t max_len, const GatherQuery& q, uint32_t threshold, GatherRow* rows_host,
                    uint32_t capacity, uint32_t* assigned_host, Device& dev, hipStream_t s);

// --- angular_kernels.hip ---------------------------------------------------------------
// Angular similarity on abundances (the rules are in include/sourmash_amd.h).  Sketches as CSR with one
// u32 abundance per hash; norm2[i] = sum of the squares of sketch i's abundances.
struct AngularSet {
  const uint64_t* hashes = nullptr;
  const uint32_t* abunds = nullptr;
  const uint64_t* offsets = nullptr;   // n+1 entries (device)
  const uint64_t* norm2 = nullptr;     // n entries (device), from launch_angular_norms
  uint32_t n = 0;
};
struct AngularOut {                    // row-major rows x cols, device memory, any may be null
  uint64_t* dot = nullptr;
  double* cosine = nullptr;
  double* angular = nullptr;
};
constexpr uint32_t kAngularNoError = 0xffffffffu;   // what an error word holds before the launches that may lower it
// abundances of a device-resident sketch -> u32: u64 counts, or differences of run starts (the two forms of DeviceSketch and
// GatherQuery); a value of 2^32 or more lowers *err_dev to err_value
void launch_angular_narrow(const uint64_t* counts, const uint32_t* starts, uint32_t total, uint32_t n, uint32_t* out,
                           uint32_t* err_dev, uint32_t err_value, hipStream_t s);
// norm2_dev[i] for every sketch; one that does not fit 64 bits lowers *err_dev to its index (the lowest one wins)
void launch_angular_norms(const uint32_t* abunds, const uint64_t* offsets_dev, uint32_t n, uint64_t* norm2_dev, uint32_t* err_dev,
                          hipStream_t s);
// prune_dev (nullable): row-major u64 matrix, a pair whose entry is 0 is not walked and gets the zero outputs.  symmetric:
// rows and cols are one set -- only col > row is walked and mirrored, the diagonal is dot = norm2, cosine = angular = 1
// (0 for an empty sketch).  counters_dev: two u64 zeroed here, [0] pairs walked, [1] pairs given zeros without a walk.
void launch_angular_block(const AngularSet& rows, const AngularSet& cols, const uint64_t* prune_dev, bool symmetric,
                          const AngularOut& out, unsigned long long* counters_dev, Device& dev, hipStream_t s);
uint32_t angular_chunk(uint32_t n_rows, uint32_t n_cols);   // columns per workgroup that launch_angular_block gives a block

// --- downsample_kernels.hip ------------------------------------------------------------
// Cutting scaled sketches at a smaller max_hash: the kept prefix of every segment of a CSR.
constexpr uint32_t kDownsampleTile = 4096;      // output elements per workgroup of the copy
constexpr uint32_t kDownsampleThreads = 256;
void downsample_geometry(uint32_t* tile_elems, uint32_t* threads);
// kept_dev[i] = how many hashes of sketch i are <= max_hash (one wave per sketch; profile name downsample_bounds)
void launch_downsample_bounds(const uint64_t* hashes, const uint64_t* offsets_dev, uint32_t n, uint64_t max_hash, uint32_t* kept_dev,
                              Device& dev, hipStream_t s);
// out[new_offsets[i] + t] = in[src_offsets[i] + t] for t < new_offsets[i + 1] - new_offsets[i]: hashes, and abundances when
// `abunds` is given.  total = new_offsets[n]; new_offsets[0] == 0.  Outputs must not alias inputs (downsample_copy).
void launch_downsample_copy(const uint64_t* hashes, const uint32_t* abunds, const uint64_t* src_offsets_dev,
                            const uint64_t* new_offsets_dev, uint32_t n, uint64_t total, uint64_t* out_hashes, uint32_t* out_abunds,
                            Device& dev, hipStream_t s);
// one device-resident sketch: out2_dev[0] = cut = how many of uniq[0 .. n) are <= max_hash, out2_dev[1] = the total its kept
// run starts end at (starts[cut], or `total` when everything is kept); without run starts out2_dev[1] = cut
void launch_downsample_cut(const uint64_t* uniq, uint64_t n, const uint32_t* starts, uint64_t total, uint64_t max_hash, uint64_t* out2_dev,
                           hipStream_t s);

// --- match_kernels.hip -----------------------------------------------------------------
// Matching records against a resident index (the rules are in include/sourmash_amd.h, "Matching records").
constexpr uint32_t kMatchSamples = 4096;          // sampled top of the directory's hashes in the probe: 32 KiB of LDS per workgroup
constexpr uint32_t kMatchLdsPairs = 1024;         // owner pairs of one record that the LDS regime of the tally takes
constexpr uint32_t kMatchThreadsPerRecord = 64;   // the tally gives a record one wave
constexpr uint32_t kMatchMiss = 0xffffffffu;      // rank of a hash no node holds; `best` of a record without hits
struct MatchRow { uint32_t windows, distinct, hit_windows, hit_distinct, best, best_common; };   // SmhMatchRow
// The hash directory of an index in device memory: U[0 .. n_hashes) the sorted distinct hashes of all nodes, the nodes
// holding U[g] are owners[starts[g] .. starts[g + 1]) ascending (the last list ends at n_pairs = the index's elements).
struct MatchDirectory {
  const uint64_t* U = nullptr;
  const uint32_t* starts = nullptr;
  const uint32_t* owners = nullptr;
  uint32_t n_hashes = 0, n_pairs = 0;
};
void match_geometry(uint32_t* lds_pairs, uint32_t* threads_per_record, uint32_t* probe_samples);
// ids[t] = the node holding element t of the CSR (t counted from offsets[0]), total = its elements
void launch_match_owner_ids(const uint64_t* offsets_dev, uint32_t n, uint64_t total, uint32_t* ids, Device& dev, hipStream_t s);
// The runs of one fold (run i: hash run_hash[i] of record run_rec[i], candidates run_start[i] .. run_start[i + 1], the last
// one ends at ncand; ordered by record, then hash) -> rank_out[i] = rank in d.U or kMatchMiss, hit_flag[i] (nullable) = 0 / 1,
// and per record r - rec0 of the fold: the first four fields of rows (zeroed by the caller) summed up, rec_first = its first
// run (caller: 0xff bytes), rec_pairs = the owners of its hit runs added up (caller: zeroed).  Profile name match_probe.
void launch_match_probe(const MatchDirectory& d, const uint64_t* run_hash, const uint64_t* run_rec, const uint32_t* run_start,
                        uint32_t nruns, uint32_t ncand, uint32_t rec0, MatchRow* rows, uint32_t* rec_first,
                        unsigned long long* rec_pairs, uint32_t* rank_out, uint32_t* hit_flag, Device& dev, hipStream_t s);
// best / best_common of every record of the fold with at most kMatchLdsPairs owner pairs (and of those without a hit); the
// others are appended to big_list (room for nrec entries; any order), *big_count (caller: zeroed) counts them.  match_tally.
void launch_match_tally(const MatchDirectory& d, const uint32_t* rank, MatchRow* rows, const uint32_t* rec_first,
                        const unsigned long long* rec_pairs, uint32_t nrec, uint32_t* big_list, uint32_t* big_count, Device& dev,
                        hipStream_t s);
// one round of the dense regime: records big[0 .. nbig) of the fold, slab = room for nbig * n_nodes counters.  match_tally.
void launch_match_dense(const MatchDirectory& d, const uint32_t* rank, MatchRow* rows, const uint32_t* rec_first, const uint32_t* big,
                        uint32_t nbig, uint32_t n_nodes, uint32_t* slab, Device& dev, hipStream_t s);
// out[at[i]] = run_hash[i] for every hit run (at: the exclusive scan of the hit flags)
void launch_match_hit_scatter(const uint64_t* run_hash, const uint32_t* rank, const uint32_t* at, uint32_t nruns, uint64_t* out, Device& dev,
                              hipStream_t s);

// --- gather_many_kernels.hip -----------------------------------------------------------
// Gather of a batch of queries through the hash directory (the rules are in include/sourmash_amd.h,
// smh_index_gather_many).  A chunk is a run of consecutive queries; its positions are those of its queries one after another.
struct GatherManyQuery { uint32_t done, rounds, best, cap; };   // cap: the rows this query may write (set by the host)
struct GatherManyState {
  uint32_t live;         // queries of the chunk that are not done (set by the host to the chunk's queries)
  uint32_t max_rounds;   // the largest number of rows any query has written
  unsigned long long hits;   // (query position, node) pairs of the chunk
};
struct GatherManyChunk {
  const uint64_t* hashes = nullptr;   // T hashes: the chunk's queries one after another, ascending strictly inside a query
  const uint64_t* counts = nullptr;   // T abundances, or null (1 each)
  const uint32_t* qoff = nullptr;     // nq + 1: where each query starts among the T positions
  uint32_t nq = 0, T = 0, n = 0;      // queries, positions, nodes of the index
  uint32_t* rank = nullptr;           // T: the position's rank in the directory or kMatchMiss
  uint32_t* c0 = nullptr;             // nq x n: |Q_q ^ S_i| (zeroed by the caller before the probe)
  uint32_t* c = nullptr;              // nq x n: the round counters (zeroed by the caller before the fill, which leaves c == c0)
  uint32_t* loff = nullptr;           // nq x n + 1: where the hit list of (query, node) starts in `lists`
  uint32_t* lists = nullptr;          // `hits` positions
  uint32_t* assigned = nullptr;       // T (caller: 0xff bytes)
  const uint64_t* rowoff = nullptr;   // nq: where each query's rows start in `rows`
  GatherRow* rows = nullptr;
  GatherManyQuery* qs = nullptr;      // nq
  GatherManyState* st = nullptr;
};
// rank, c0 and st->hits of the chunk, then qcnt[q] = the nodes with c0 >= threshold.  Profile name gather_many_probe.
void launch_gather_many_probe(const MatchDirectory& d, const GatherManyChunk& ck, uint32_t threshold, uint32_t* qcnt, Device& dev,
                              hipStream_t s);
// loff (the scan of c0) and the hit lists; c counts up to c0 on the way.  Profile name gather_many_fill.
void launch_gather_many_fill(const MatchDirectory& d, const GatherManyChunk& ck, Device& dev, hipStream_t s);
// `rounds` rounds of every query of the chunk: 2 launches each.  node_offsets: the index's CSR offsets (size_match);
// sub_grid: workgroups per query of the subtract.  Profile name gather_many_rounds (one entry per call).
void launch_gather_many_rounds(const MatchDirectory& d, const GatherManyChunk& ck, const uint64_t* node_offsets, uint32_t threshold,
                               uint32_t sub_grid, uint32_t rounds, Device& dev, hipStream_t s);
// out[p] = the abundance of position p of a device-resident sketch held as run starts (the last run ends at total); starts
// null: 1 each
void launch_gather_many_weights(const uint32_t* starts, uint32_t total, uint32_t n, uint64_t* out, hipStream_t s);

// --- search_many_kernels.hip -----------------------------------------------------------
// The (query, node) pairs of a batch of queries over a threshold (the rules are in include/sourmash_amd.h,
// smh_index_search_many).  A chunk is a run of consecutive queries, as gather_many's.
constexpr uint32_t kSearchTile = 1024;           // nodes of one workgroup of the select and emit kernels (256 threads, 4 nodes each)
constexpr uint32_t kSearchMaxQueries = 65535;    // queries per chunk: the second dimension of their grid
enum SearchMetric : uint32_t { kSearchJaccard = 0, kSearchContainmentNode = 1, kSearchContainmentQuery = 2, kSearchMaxContainment = 3 };
enum SearchSelf : uint32_t { kSearchNotSelf = 0, kSearchNoDiagonal = 1, kSearchUpperOnly = 2 };
struct SearchRow { uint32_t node, common, node_size, query_size; };   // SmhSearchRow
struct SearchChunk {
  const uint64_t* hashes = nullptr;        // T hashes: the chunk's queries one after another, ascending strictly inside a query
  const uint32_t* qoff = nullptr;          // nq + 1: where each query starts among the T positions
  uint32_t nq = 0, T = 0, n = 0;           // queries, positions, nodes of the index
  uint32_t q0 = 0;                         // self modes: the node that the chunk's first query is
  uint32_t* c = nullptr;                   // nq x n: |Q_q ^ S_i| (zeroed by the caller before the probe)
  uint32_t* tile_rows = nullptr;           // nq x tiles + 1: survivors per (query, tile); after the scan where each tile's rows start
  uint32_t tiles = 0;                      // ceil(n / kSearchTile)
  const uint64_t* node_offsets = nullptr;  // the index's CSR offsets in device memory (|S_i|)
  uint32_t metric = 0, self = 0, threshold_common = 1;
  double threshold = 0;
};
void search_geometry(uint32_t* short_owners, uint32_t* node_tile, uint32_t* max_queries);
// c of the chunk.  Profile name search_many_probe.
void launch_search_many_probe(const MatchDirectory& d, const SearchChunk& ck, Device& dev, hipStream_t s);
// tile_rows counted and scanned in place: tile_rows[nq * tiles] is the chunk's rows.  Profile name search_many_select.
void launch_search_many_select(const SearchChunk& ck, Device& dev, hipStream_t s);
// the chunk's rows in order (query, then node), and query_rows[q] = where the rows of query q start.  Profile name
// search_many_emit.
void launch_search_many_emit(const SearchChunk& ck, SearchRow* rows, uint32_t* query_rows, Device& dev, hipStream_t s);

// --- nearest_kernels.hip ---------------------------------------------------------------
// The best k rows of every query by (value descending, node ascending) (the rules are in
// include/sourmash_amd.h, smh_index_nearest_many).  A chunk is search_many's, and so is its front half: these come behind
// launch_search_many_select.
constexpr uint32_t kNearestMaxK = 256;           // the largest k: a merge step then still takes kNearestSlots - 256 candidates
constexpr uint32_t kNearestSlots = 1024;         // keys the merge sorts in LDS at once (12 KiB); a tile's survivors fit them
struct NearestChunk {
  uint32_t k = 0;
  uint32_t* cand_at = nullptr;   // nq x tiles + 1: candidates kept per (query, tile); after the scan where each tile's start
  uint32_t* row_at = nullptr;    // = cand_at + nq x tiles + 1; nq + 1: rows per query; after the scan row_at[q] - row_at[0] is where
                                 // query q's rows start (one scan runs over both arrays: row_at[0] is the chunk's candidates)
  uint64_t* cand_v = nullptr;    // per kept candidate: the value's bits ...
  uint32_t* cand_n = nullptr;    // ... and the node
};
void nearest_geometry(uint32_t* max_k, uint32_t* node_tile, uint32_t* merge_slots);
// cand_at and row_at from ck.tile_rows (scanned), scanned in place as one array: cand_at[nq * tiles] is the chunk's
// candidates, row_at[nq] its candidates + its rows.  Profile name nearest_clamp.
void launch_nearest_clamp(const SearchChunk& ck, const NearestChunk& nc, Device& dev, hipStream_t s);
// every tile's best candidates, in order, at its place in cand_v / cand_n.  Profile name nearest_tile.
void launch_nearest_tile(const SearchChunk& ck, const NearestChunk& nc, Device& dev, hipStream_t s);
// the chunk's rows: query q's at row_at[q] - row_at[0], in order.  Profile name nearest_merge.
void launch_nearest_merge(const SearchChunk& ck, const NearestChunk& nc, SearchRow* rows, Device& dev, hipStream_t s);

// --- cluster_kernels.hip ---------------------------------------------------------------
// Clustering a resident index (the rules are in include/sourmash_amd.h, smh_index_cluster).  Components: the
// upper triangle of a chunk's counters is probed and every survivor of the rule is a union; greedy: the rows of the search
// kernels stay in HBM as adjacency lists and synchronous rounds decide the representatives.
enum ClusterLinkage : uint32_t { kClusterComponents = 0, kClusterGreedy = 1 };
enum ClusterState : uint32_t { kClusterUndecided = 0, kClusterRep = 1, kClusterMember = 2 };
constexpr uint32_t kClusterLaneMax = 16;         // adjacency lists up to this length are walked by the lane that holds the node
constexpr uint32_t kClusterRoundsPerSync = 32;   // greedy rounds queued between two read-backs (kGatherRoundsPerSync's choice)
struct ClusterAdj { uint32_t node, common; };    // one directed adjacency entry: the neighbour and |S_v ^ S_node|
void cluster_geometry(uint32_t* lane_max, uint32_t* node_tile);
// v[i] = i
void launch_cluster_iota(uint32_t* v, uint32_t n, hipStream_t s);
// the chunk's counters of the pairs with owner > query only (ck.q0 = the node that the chunk's first query is; c zeroed by the
// caller).  Profile name cluster_probe.
void launch_cluster_probe(const MatchDirectory& d, const SearchChunk& ck, Device& dev, hipStream_t s);
// uf_union(parent, query, node) for every survivor of the rule under kSearchUpperOnly.  Profile name cluster_link.
void launch_cluster_link(const SearchChunk& ck, uint32_t* parent, Device& dev, hipStream_t s);
// Components, finishing pass.  scores (nullable: |S_v| from node_offsets); work: room for 4 n + 2 u32 (8-byte aligned);
// out: cluster[n], representative[n], then the number of clusters.  Profile name cluster_finish.
void launch_cluster_finish_components(uint32_t* parent, const uint32_t* scores, const uint64_t* node_offsets, uint32_t n, uint32_t* work,
                                      uint32_t* out, Device& dev, hipStream_t s);
// adj[base + k] = {rows[k].node, rows[k].common} for the R rows of a chunk, and start[q] = base + query_rows[q] for its nq
// queries (query_rows null: the chunk has no rows, start[q] = base)
void launch_cluster_pack(const SearchRow* rows, uint32_t R, const uint32_t* query_rows, uint32_t nq, uint32_t base, ClusterAdj* adj,
                         uint32_t* start, hipStream_t s);
// One synchronous round: st_out from st_in (ClusterState per node), start: n + 1 entries.  undecided (nullable): += the nodes
// still undecided in st_out.
void launch_cluster_round(const uint32_t* start, const ClusterAdj* adj, const uint32_t* rank, const uint32_t* st_in, uint32_t* st_out,
                          uint32_t n, unsigned long long* undecided, Device& dev, hipStream_t s);
// Greedy, members and numbering.  work: room for 2 n + 1 u32; out: cluster[n], representative[n], rep_common[n], then the
// number of clusters.  Profile names cluster_assign, cluster_finish.
void launch_cluster_assign(const uint32_t* start, const ClusterAdj* adj, const uint32_t* rank, const uint32_t* st, uint32_t metric,
                           const uint64_t* node_offsets, uint32_t n, uint32_t* work, uint32_t* out, Device& dev, hipStream_t s);

// --- lca_kernels.hip -------------------------------------------------------------------
// Taxonomic LCA on a resident index (the rules are in include/sourmash_amd.h, "Taxonomic LCA").
constexpr uint32_t kLcaNoTaxon = 0xffffffffu;    // SMH_NO_TAXON: a node without a lineage, an unassigned hash, an empty set
constexpr uint32_t kLcaOwnerLaneMax = 8;         // owner lists up to this length are folded by one lane of the table kernel
constexpr uint32_t kLcaRecordLaneMax = 8;        // records with up to this many runs are folded by one lane
constexpr uint32_t kLcaThreads = 64;             // what a longer owner list / record gets: one wave
struct LcaRow { uint32_t windows, distinct, hit_distinct, assigned_distinct, taxon, status; };   // SmhLcaRow
// The taxonomy in device memory: tax[t] = {parent, depth} (8 bytes, one load per step of the walk), node_taxon[i] = the
// taxon of node i or kLcaNoTaxon.
struct LcaTaxonomy {
  const uint64_t* tax = nullptr;   // read as uint2 {parent, depth}
  const uint32_t* node_taxon = nullptr;
};
void lca_geometry(uint32_t* owner_lane_max, uint32_t* record_lane_max, uint32_t* threads);
// hash_taxon[g] for every rank g of the directory.  long_list: room for n_pairs / (kLcaOwnerLaneMax + 1) + 1 entries,
// long_count: one word (zeroed here).  Profile name lca_table.
void launch_lca_table(const MatchDirectory& d, const LcaTaxonomy& t, uint32_t* hash_taxon, uint32_t* long_list, uint32_t* long_count,
                      Device& dev, hipStream_t s);
// The T positions of a chunk of nq queries (qoff: nq + 1 offsets among them; hashes ascend strictly inside a query):
// taxon_out[p] = the taxon of hash p or kLcaNoTaxon, key_out[p] = (query << 32) | taxon, flag_out[p] = 1 for an assigned
// hash.  Profile name lca_probe.
void launch_lca_probe(const MatchDirectory& d, const uint32_t* hash_taxon, const uint64_t* hashes, const uint32_t* qoff, uint32_t nq,
                      uint32_t T, uint32_t* taxon_out, uint64_t* key_out, uint32_t* flag_out, Device& dev, hipStream_t s);
// out[at[p]] = key[p] for every assigned position (at: the exclusive scan of the flags)
void launch_lca_keys(const uint64_t* key, const uint32_t* at, uint32_t T, uint64_t* out, Device& dev, hipStream_t s);
// The rows of a fold's nrec records after launch_match_probe (rows, rec_first, rank as it left them) -> out.  big_list: room
// for nrec entries, big_count: one word (zeroed here).  Profile name lca_records.
void launch_lca_records(const LcaTaxonomy& t, const uint32_t* hash_taxon, const uint32_t* rank, const MatchRow* rows,
                        const uint32_t* rec_first, uint32_t nrec, LcaRow* out, uint32_t* big_list, uint32_t* big_count, Device& dev,
                        hipStream_t s);

// --- collapse_kernels.hip --------------------------------------------------------------
// Collapsing a resident index by groups (the rules are in include/sourmash_amd.h, "Collapsing an index by
// groups").  The owner list of every rank of the hash directory is folded through group[] to the groups that hold the hash
// often enough; a survivor is one (group, rank) with its count or abundance sum.
enum CollapseAbund : uint32_t { kCollapseFlat = 0, kCollapseSum = 1, kCollapseCount = 2 };
constexpr uint32_t kCollapseDrop = 0xffffffffu;    // SMH_COLLAPSE_DROP: a node that takes no part
constexpr uint32_t kCollapseNoError = 0xffffffffu; // what the error word holds before the emit pass may lower it
constexpr uint32_t kCollapseLaneMax = 8;           // owner lists up to this length are folded by the lane that holds the rank (kLcaOwnerLaneMax's choice)
constexpr uint32_t kCollapseWaveMax = 256;         // ... up to this length by one wave, the owners' groups in its LDS scratch (1 KiB per wave)
constexpr uint32_t kCollapseGroupTile = 2048;      // longer lists: one workgroup, LDS counters over this many groups at a time (8 KiB, 24 with sums)
struct CollapseFold {
  MatchDirectory d;
  const uint32_t* group = nullptr;     // n entries: the node's group or kCollapseDrop
  const uint32_t* need = nullptr;      // n_groups entries: need_g
  uint32_t n_groups = 0;
  uint32_t* cnt = nullptr;             // n_hashes + 1: survivors per rank; scanned in place between the passes (the last entry: their total)
  uint32_t* wave_list = nullptr;       // ranks with more than kCollapseLaneMax owners: room for n_pairs / (kCollapseLaneMax + 1) + 1 ...
  uint32_t* long_list = nullptr;       // ... and with more than kCollapseWaveMax: n_pairs / (kCollapseWaveMax + 1) + 1
  uint32_t* list_count = nullptr;      // two words, [0] wave_list's, [1] long_list's (zeroed by the count pass)
  // the emit pass
  uint32_t abund = kCollapseFlat;
  const uint64_t* hashes = nullptr;    // kCollapseSum: the index's CSR and its abundances in device memory
  const uint64_t* offsets = nullptr;
  const uint32_t* abunds = nullptr;
  uint64_t* key = nullptr;             // per survivor (group << 32) | rank
  uint32_t* val = nullptr;             // per survivor c_g(h) or a_g(h); null under kCollapseFlat
  uint32_t* err = nullptr;             // kCollapseSum: atomicMin of the groups holding a kept sum of 2^32 or more (caller: 0xff bytes)
};
void collapse_geometry(uint32_t* lane_max, uint32_t* wave_max, uint32_t* group_tile);
// cnt and the two lists.  Profile name collapse_count.
void launch_collapse_count(const CollapseFold& f, Device& dev, hipStream_t s);
// key / val of every survivor, those of rank r at cnt[r] .. cnt[r + 1] (cnt scanned; any order inside a rank: a group appears
// once there).  Reads the lists the count pass left.  Profile name collapse_emit.
void launch_collapse_emit(const CollapseFold& f, Device& dev, hipStream_t s);
// start[g] = how many of the S partitioned keys belong to groups below g, for g = 0 .. n_groups (n_groups + 1 entries)
void launch_collapse_bounds(const uint64_t* key, uint32_t S, uint32_t n_groups, uint32_t* start, Device& dev, hipStream_t s);
// out_hashes[i] = U[rank of key[i]], out_abunds[i] = val[i] (both nullable together) for the S partitioned survivors.  Profile
// name collapse_finish.
void launch_collapse_finish(const uint64_t* U, const uint64_t* key, const uint32_t* val, uint32_t S, uint64_t* out_hashes,
                            uint32_t* out_abunds, Device& dev, hipStream_t s);

// --- index_build_kernels.hip -----------------------------------------------------------
// Building an index from records (the rules are in include/sourmash_amd.h, "Building an index from records").
// The candidates of a fold, sorted by (group, hash), become runs -- one per distinct (group, hash) -- without a host pass:
// heads are counted per tile, the counts are scanned, and an ordered emit numbers the heads.  An element is (hash, tag):
// its group is tag >> shift, and with shift == kBuildCountBits the bits below hold a count (a run of an earlier fold).
constexpr uint32_t kBuildTile = 2048;        // candidates per workgroup of the head and emit passes (256 threads, 8 each)
constexpr uint32_t kBuildThreads = 256;
constexpr int kBuildCountBits = 40;          // a packed run: (group << 40) | count; groups stay below 2^24 (the grouped path's limit)
constexpr uint32_t kBuildNoError = 0xffffffffu;
void index_build_geometry(uint32_t* tile_elems, uint32_t* threads);
inline uint32_t index_build_tiles(uint64_t n) { return (uint32_t)((n + kBuildTile - 1) / kBuildTile); }
// out[i] = groups ? groups[i / per] : i / per, for i < n_entries (per = 6: the segments of the translated arm)
void launch_index_build_groups(const uint32_t* groups, uint64_t n_entries, uint32_t per, uint32_t* out, hipStream_t s);
// tile_heads[t] = the heads among elements [t * kBuildTile, ...) of the n sorted elements.  Profile name index_build_heads.
void launch_index_build_heads(const uint64_t* hash, const uint64_t* tag, uint64_t n, int shift, uint32_t* tile_heads, Device& dev,
                              hipStream_t s);
// tile_heads scanned (exclusive): run_hash[r] and run_start[r] of every head, in order.  Profile name index_build_emit.
void launch_index_build_emit(const uint64_t* hash, const uint64_t* tag, uint64_t n, int shift, const uint32_t* tile_heads,
                             uint64_t* run_hash, uint32_t* run_start, Device& dev, hipStream_t s);
// run_pack[r] = (group << kBuildCountBits) | count of run r = elements [run_start[r], run_start[r + 1]) (the last ends at n):
// their number under shift == 0, else the sum of their counts.  A count of 2^32 or more lowers *err to the run's group (the
// word then holds the low 32 bits).  Belongs to the emit pass's timer.
void launch_index_build_counts(const uint64_t* tag, uint64_t n, int shift, const uint32_t* run_start, uint32_t nruns, uint64_t* run_pack,
                               uint32_t* err, Device& dev, hipStream_t s);
// The n_runs packed runs, ascending by group: offsets[g] = base + the runs of the groups below g, for g = 0 .. n_groups (one
// bisecting lane per group), and abunds[r] (nullable) = the count of run r.
void launch_index_build_finish(const uint64_t* run_pack, uint32_t n_runs, uint32_t n_groups, uint64_t* offsets, uint32_t* abunds, Device& dev,
                               hipStream_t s);
// dst[i] = src[i] + delta for i < n (the offsets of a part of a concatenation; delta wraps like the subtraction it stands for)
void launch_index_build_rebase(const uint64_t* src, uint64_t n, uint64_t delta, uint64_t* dst, hipStream_t s);

// --- filter_kernels.hip ----------------------------------------------------------------
// Filtering a resident index (the rules are in include/sourmash_amd.h, "Filtering an index"): a verdict per
// resident hash, then an ordered compaction per node.  Element t of the index is hashes[t] (the caller passes the CSR from
// offsets[0] on); a tile is kFilterTile consecutive elements and may span any number of nodes.
enum FilterOperand : uint32_t { kFilterOperandNone = 0, kFilterKeepIn = 1, kFilterDropIn = 2 };
enum FilterAbund : uint32_t { kFilterAbundOwn = 0, kFilterAbundFlat = 1, kFilterAbundOperand = 2 };
constexpr uint32_t kFilterTile = 2048;        // elements per workgroup trip of the flag and emit passes (256 threads, 8 each)
constexpr uint32_t kFilterThreads = 256;
constexpr uint32_t kFilterSamples = 2048;     // sampled top of the operand's hashes: 16 KiB of LDS per workgroup
constexpr uint32_t kFilterWords = kFilterTile / 64;   // mask words of a tile: one per wave and step
struct FilterRule {                           // SmhFilter
  uint32_t operand_mode, abund_out, min_abund, max_abund, min_owners, max_owners;
  __host__ __device__ bool abund_window() const { return !(min_abund == 0 && max_abund == 0xffffffffu); }
  __host__ __device__ bool owner_window() const { return !(min_owners <= 1 && max_owners == 0xffffffffu); }
};
struct FilterPass {
  const uint64_t* hashes = nullptr;      // total elements
  const uint32_t* abunds = nullptr;      // total abundances: the window's and OWN's; null when neither is asked
  uint64_t total = 0;
  const uint64_t* operand = nullptr;     // n_operand ascending distinct hashes (operand_mode != NONE)
  const uint32_t* operand_abunds = nullptr;   // OPERAND: one per operand hash
  uint32_t n_operand = 0;
  MatchDirectory dir;                    // the owner window's; read only when the rule has one
  FilterRule rule;
  uint64_t* mask = nullptr;              // filter_tiles(total) * kFilterWords words: bit t = element t is kept
  uint64_t* tile_at = nullptr;           // filter_tiles(total) + 1: survivors per tile; scanned in place (exclusive, the last: their total)
};
void filter_geometry(uint32_t* tile, uint32_t* operand_samples, uint32_t* threads);
inline uint64_t filter_tiles(uint64_t total) { return (total + kFilterTile - 1) / kFilterTile; }
// mask and tile_at (counts) of every tile.  Profile name filter_flag.
void launch_filter_flag(const FilterPass& f, Device& dev, hipStream_t s);
// tile_at[0 .. tiles] scanned in place, 64 bits wide: one workgroup, a carry from block to block
void launch_filter_scan(uint64_t* tile_at, uint64_t tiles, hipStream_t s);
// new_off[i] = the survivors in front of element offsets[i] - offsets[0], for i = 0 .. n (one lane per node)
void launch_filter_offsets(const FilterPass& f, const uint64_t* offsets_dev, uint32_t n, uint64_t* new_off, Device& dev, hipStream_t s);
// the survivors in order: out_hashes, and out_abunds (nullable) from f.abunds (OWN) or f.operand_abunds (OPERAND: the
// operand is searched again for the survivors).  Profile name filter_emit.
void launch_filter_emit(const FilterPass& f, uint64_t* out_hashes, uint32_t* out_abunds, Device& dev, hipStream_t s);

}  // namespace smh
