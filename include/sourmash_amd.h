/*
 * include/sourmash_amd.h -- ADDITIVE entry points of the MI355X implementation.
 *
 * The reference ABI (sourmash.h) hands the library one NUL-terminated C string and one pair of
 * sketches per call.  These symbols add what a GPU needs: explicit lengths, many records per
 * call, device-resident buffers, and an N x M compare block.  None of them changes or shadows
 * a reference symbol.  Plain pointers and sizes only; `stream` is a hipStream_t passed as
 * void*.  NULL = the library's own stream, which is first ordered after everything already queued
 * on the legacy default stream (where a caller without streams of its own produced the inputs);
 * every entry point returns with its device work complete -- with three stated exceptions.  Two are
 * smh_collection_begin with world == 1 and smh_collection_finish without a gathered buffer (a single
 * owner's dictionary, which only later calls of this library use): their work is left queued, and
 * EVERY later entry point, on whatever stream it is given, is first ordered behind it (an event
 * recorded behind the open work; the library's shared scratch buffers are never rewritten under it).
 * The third is smh_synth_dna_dev with a caller's stream: its one kernel is left queued on that stream
 * and touches nothing but the caller's buffer, so work the caller queues behind it on the SAME stream
 * (a sketching call given that stream) reads the finished bytes; anything else waits for the stream
 * first.  With NULL it waits like every other call.
 * "dev" pointers are HIP device pointers.
 *
 * Error convention: same thread-local slot as sourmash.h; functions returning int return 0 on
 * success and the SourmashErrorCode otherwise.
 */
#ifndef SOURMASH_AMD_H_INCLUDED
#define SOURMASH_AMD_H_INCLUDED

#include "sourmash.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when a HIP device can be used, 0 otherwise (never raises). */
int smh_device_available(void);
/* device ordinal in use and its compute-unit count (0 on failure, error slot set) */
int smh_device_info(int *device, int *compute_units);

/* KmerMinHash::add_sequence (reference src/lib.rs:252-305) with an explicit length: the bytes
 * may contain NUL.  Same semantics and errors as kmerminhash_add_sequence. */
int smh_add_sequence_len(KmerMinHash *ptr, const char *seq, uint64_t len, bool force);

/* Many records in one call, as if add_sequence were called on each in order
 * (offsets: n_records+1 host entries into seq).  Every record is processed; the first record
 * that the reference would have failed on is the reported error.  *_dev: seq is a device
 * pointer (inputs already resident in HBM). */
int smh_add_sequences(KmerMinHash *ptr, const char *seq, const uint64_t *offsets,
                      uint32_t n_records, bool force);
int smh_add_sequences_dev(KmerMinHash *ptr, const void *seq_dev, uint64_t total_len,
                          const uint64_t *offsets, uint32_t n_records, bool force, void *stream);

/* Many sketches from one batch: record r feeds sketches[groups[r]] (one genome = one group of
 * contigs; the loop of reference src/lib.rs:252-305 callers that build one signature per input
 * file).  Per sketch the result is that of smh_add_sequences over its records in order.  Sketches
 * of one molecule type with equal (ksize, seed) share ONE hashing launch and ONE sort when they
 * are all scaled with one max_hash, or (DNA) all bottom-num; other
 * parameter combinations are served sketch by sketch. */
int smh_add_sequences_grouped(KmerMinHash *const *sketches, uint32_t n_sketches, const char *seq,
                              const uint64_t *offsets, const uint32_t *groups, uint32_t n_records, bool force);
int smh_add_sequences_grouped_dev(KmerMinHash *const *sketches, uint32_t n_sketches, const void *seq_dev,
                                  uint64_t total_len, const uint64_t *offsets, const uint32_t *groups,
                                  uint32_t n_records, bool force, void *stream);

/* Records cut out of FASTA / FASTQ text ON THE DEVICE: the text, resident in HBM, becomes the layout the
 * entry points above take -- one dense buffer of sequence bytes plus n+1 offsets -- without a host pass over lines.
 *   Lines      end at '\n'; one '\r' directly in front of it, or a '\r' that is the text's last byte, belongs to the
 *              terminator; every other byte belongs to the line.  A line is empty when nothing but the terminator is left.
 *   FASTA      a line whose first byte is '>' starts a record; its sequence is every following non-header line up to the
 *              next header, terminators removed; empty lines are ignored; a header followed by a header or by the end of
 *              the text is a record of length 0.  A non-empty non-header line in front of the first header is an error
 *              (code 3, the message names its byte offset).
 *   FASTQ      strict four-line records ('@' line, sequence, '+' line, quality of the sequence's length); the line number
 *              alone decides a line's role.  Empty lines at the end of the text are dropped; after that a last record of
 *              three lines whose sequence line is empty is complete.  Anything else is an error (code 3); the message
 *              names the lowest malformed record in file order as "record N", 0-based.
 *   AUTO       the first byte of the first non-empty line decides: '>' FASTA, '@' FASTQ, anything else is an error.
 * Sequence bytes are passed on untouched (lower case, N, IUPAC codes, a stray '\r'): what they mean is add_sequence's
 * business, exactly as if the caller had cut the records by hand.  The handle owns the compacted bytes (device), the
 * offsets (host) and the name spans; it keeps NO reference to the text, which may be freed when the parse returns.
 * A record's name is its header line without the marker byte and the terminator, reported as a span (start, length)
 * INTO THE TEXT: the library copies no names.  smh_records_parse uploads host text and parses it; *_parse_dev takes
 * text already in HBM (any alignment).  More than 2^32 - 1 records in one text is an error at parse time.
 * smh_add_records / smh_add_records_grouped give the result of smh_add_sequences_dev / smh_add_sequences_grouped_dev
 * on the same records; groups == NULL: record i feeds sketches[i] and n_sketches must equal the number of records. */
typedef struct SmhRecords SmhRecords;
enum { SMH_FORMAT_AUTO = 0, SMH_FORMAT_FASTA = 1, SMH_FORMAT_FASTQ = 2 };
SmhRecords *smh_records_parse(const char *text, uint64_t len, int format);
SmhRecords *smh_records_parse_dev(const void *text_dev, uint64_t len, int format, void *stream);
void smh_records_free(SmhRecords *r);
uint32_t smh_records_len(const SmhRecords *r);
uint64_t smh_records_total(const SmhRecords *r);          /* kept sequence bytes */
int smh_records_format(const SmhRecords *r);              /* what AUTO resolved to */
const void *smh_records_seq_dev(const SmhRecords *r);     /* the compacted bytes, device */
const uint64_t *smh_records_offsets(const SmhRecords *r); /* n+1 host entries, valid while the handle lives */
int smh_records_names(const SmhRecords *r, uint64_t *start_out, uint32_t *len_out);   /* n entries each */
uint32_t smh_records_tile_bytes(void);                    /* bytes per workgroup tile of the parser (tests, tools) */
int smh_add_records(KmerMinHash *ptr, const SmhRecords *r, bool force);
int smh_add_records_grouped(KmerMinHash *const *sketches, uint32_t n_sketches, const SmhRecords *r, const uint32_t *groups,
                            bool force);

/* Blocked gzip (BGZF, what bgzip / htslib write) inflated ON THE DEVICE, in front of the parser.  The file
 * is a chain of independent gzip members (RFC 1952), each at most 64 KiB compressed and at most 64 KiB inflated; a member's
 * compressed size is in its header (extra subfield 'B' 'C', SLEN 2: BSIZE = member size - 1), its CRC-32 and inflated size
 * (ISIZE) in its trailer.  The host finds every member by hopping headers; the device inflates all members at once, each
 * into its own slice of the text.  Plain single-stream gzip has no such structure and stays with the caller.
 *   smh_gzip_scan   walks the headers of data[0, len) and needs no device.  Per member: magic 1f 8b, CM 8; FEXTRA with any
 *              subfields in front of and behind BC (the first BC counts); FNAME and FCOMMENT up to their NUL; FHCRC.  It
 *              records the payload's offset and length, ISIZE, the CRC-32 and the running output offset (64 bits).  An empty
 *              input is zero members; a member with ISIZE 0 (the BGZF end marker, anywhere in the chain) is a member like
 *              any other and is decoded and checked.  Refusals are code 3 and name the member's index and byte offset as
 *              "(member I at byte B)":  "the bytes are not gzip" (member 0 without the magic or with another CM);  "not
 *              blocked gzip" (a member without BC: the caller may fall back to a host gzip);  "BSIZE runs past the end";
 *              "header is cut short" (the fixed header, XLEN, a subfield, a name without NUL, or a header and trailer
 *              that BSIZE has no room for);  "ISIZE above 65536";  "bytes trail after the last member" (anything behind a
 *              member that does not begin another).
 *   smh_gzip_member   payload offset and length, ISIZE and CRC-32 of member i (any pointer may be NULL).
 *   smh_gzip_inflate_dev   data_dev: the len scanned bytes in HBM at any alignment; out_dev receives the text, out_cap
 *              must be at least smh_gzip_inflated_len.  It follows the stream contract at the top of this file: the work is
 *              ordered on `stream` (NULL: the library's own, behind the legacy default stream) and is complete on return.
 *              verify_crc = 0 skips the CRC-32; ISIZE is always checked.  status_out (host, one byte per member, or NULL)
 *              receives every member's status, also when the call fails.  A member stops at the FIRST rule it breaks, so
 *              its status is deterministic:
 *                 0  ok
 *                 1  reserved block type (3)
 *                 2  stored block whose LEN is not the complement of NLEN
 *                 3  more than 286 literal/length codes or more than 30 distance codes announced
 *                 4  code-length repeat 16 with nothing to repeat, or a repeat running past the announced lengths
 *                 5  over-subscribed code set (code-length, literal/length or distance)
 *                 6  incomplete code set; a literal/length or distance set of ONE code of length 1, and a distance set
 *                    without any code, are legal; an incomplete code-length set never is
 *                 7  no end-of-block code (symbol 256 has length 0)
 *                 8  invalid symbol: literal/length 286 or 287, distance 30 or 31, or bits that no code of the set has
 *                 9  distance reaching in front of the member's own output
 *                10  input exhausted (a symbol is read a bit at a time: the payload ends before a code is complete)
 *                11  output would pass ISIZE
 *                12  stream ends with output below ISIZE
 *                13  payload bytes left over after the final block (bits of its last byte are not bytes)
 *                14  CRC-32 mismatch
 *              Checks happen in stream order; in a dynamic header: the counts, the code-length set, the lengths and their
 *              repeats, the end-of-block code, the literal/length set, the distance set.  A failing call returns code 3 and
 *              names the LOWEST bad member, its byte offset and the reason.  On failure the contents of out_dev are
 *              unspecified, but on ANY input no byte outside out[0, inflated_len) is written and no byte outside
 *              data[0, len) is read.  len must be the length that was scanned.
 *   smh_gzip_inflate   the same from host bytes: scans, uploads the compressed bytes once, inflates. */
typedef struct SmhGzip SmhGzip;
enum { SMH_INFLATE_OK = 0, SMH_INFLATE_BLOCK_TYPE = 1, SMH_INFLATE_STORED_LEN = 2, SMH_INFLATE_HEADER_COUNTS = 3, SMH_INFLATE_REPEAT = 4,
       SMH_INFLATE_OVER_SUBSCRIBED = 5, SMH_INFLATE_INCOMPLETE = 6, SMH_INFLATE_NO_END_OF_BLOCK = 7, SMH_INFLATE_BAD_SYMBOL = 8,
       SMH_INFLATE_DISTANCE = 9, SMH_INFLATE_INPUT = 10, SMH_INFLATE_OUTPUT_OVER = 11, SMH_INFLATE_OUTPUT_UNDER = 12,
       SMH_INFLATE_LEFTOVER = 13, SMH_INFLATE_CRC = 14 };
SmhGzip *smh_gzip_scan(const void *data, uint64_t len);
void smh_gzip_free(SmhGzip *g);
uint64_t smh_gzip_members(const SmhGzip *g);
uint64_t smh_gzip_inflated_len(const SmhGzip *g);
int smh_gzip_member(const SmhGzip *g, uint64_t i, uint64_t *payload_off, uint32_t *payload_len, uint32_t *isize, uint32_t *crc);
int smh_gzip_inflate_dev(const SmhGzip *g, const void *data_dev, uint64_t len, void *out_dev, uint64_t out_cap, int verify_crc,
                         uint8_t *status_out /* host, one per member, or NULL */, void *stream);
int smh_gzip_inflate(const void *data, uint64_t len, void *out_dev, uint64_t out_cap, int verify_crc, uint8_t *status_out);

/* Alphabets and amino-acid input.  The reference revision sketches protein only out of translated DNA
 * and in the 20-letter alphabet only; this library fixes the rest:
 *   Molecule   a sketch has one of DNA, protein, dayhoff, hp.  kmerminhash_new(prot = false / true) gives DNA / protein;
 *              kmerminhash_is_protein is true for the last three.  ksize stays in nucleotides: the window is
 *              W = ksize / 3 residues (dayhoff k = 9 is ksize 27).  Sketches of different molecules are incompatible
 *              (code 102) wherever check_compatible applies; the signature JSON's "molecule" is "DNA", "protein",
 *              "dayhoff" or "hp", the last two are read back as such (any other string still reads as DNA), and the
 *              moltype filter of the load calls matches them case-insensitively.
 *   Maps       applied to the upper-cased byte (a-z become A-Z, nothing else changes).
 *              protein  every byte is itself
 *              dayhoff  C -> a;  A G P S T -> b;  D E N Q -> c;  H K R -> d;  I L M V -> e;  F W Y -> f;  * -> *;
 *                       every other byte -> X
 *              hp       A F G I L M P V W Y -> h;  N C S T D E R H K Q -> p;  * -> *;  every other byte -> X
 *   Amino-acid input (smh_add_protein*)   for each record in order, for each start i with i + W <= len ascending:
 *              add_hash(murmur64(map(record[i .. i + W)), seed)).  No strand, no translation, no validity check, no
 *              `force`: content never raises an error, and NUL, 0xFF and bytes >= 0x80 are residues like any other.  A
 *              record shorter than W adds nothing; W == 0 raises add_sequence's panic; a DNA sketch is refused with code 3
 *              before the device is touched.  Calls take effect in call order with add_sequence / add_word / add_hash
 *              on the same sketch.  Without a usable device: code 2 and the sketch is unchanged.
 *   Translated input   add_sequence and its batch / device / grouped / records forms on a dayhoff or hp sketch behave
 *              exactly as on a protein sketch (six frames in the reference's order, unknown codons dropped, the UTF-8
 *              panic, `force` ignored); each residue is mapped before hashing ('*' stays '*').
 * smh_add_proteins* follow smh_add_sequences*: offsets has n_records + 1 host entries, seq_dev may have any alignment.
 * smh_add_records_protein feeds a parsed protein FASTA (the parser passes sequence bytes on untouched).
 * smh_amino_geometry: window starts per workgroup tile and per lane of the hashing launch for that input (tests, tools). */
enum { SMH_MOLECULE_DNA = 0, SMH_MOLECULE_PROTEIN = 1, SMH_MOLECULE_DAYHOFF = 2, SMH_MOLECULE_HP = 3 };
KmerMinHash *smh_kmerminhash_new_molecule(uint32_t n, uint32_t k, int molecule, uint64_t seed, uint64_t mx, bool track_abundance);
int smh_kmerminhash_molecule(const KmerMinHash *ptr);
int smh_add_protein(KmerMinHash *ptr, const char *seq, uint64_t len);
int smh_add_proteins(KmerMinHash *ptr, const char *seq, const uint64_t *offsets, uint32_t n_records);
int smh_add_proteins_dev(KmerMinHash *ptr, const void *seq_dev, uint64_t total_len, const uint64_t *offsets, uint32_t n_records,
                         void *stream);
int smh_add_records_protein(KmerMinHash *ptr, const SmhRecords *r);
void smh_amino_geometry(uint64_t total_len, uint32_t win, uint32_t *tile_positions, uint32_t *run);

/* add_hash over an array (reference src/lib.rs:412-417 add_many) */
int smh_add_many(KmerMinHash *ptr, const uint64_t *hashes, uint64_t n);

/* KmerMinHash::add_many_with_abund (reference src/lib.rs:419-426; Rust API only, the reference header
 * has no symbol for it): item i is the pair (hashes[i], abunds[i]) and is added abunds[i] times. */
int smh_add_many_with_abund(KmerMinHash *ptr, const uint64_t *hashes, const uint64_t *abunds, uint64_t n);

/* KmerMinHash::check_compatible (reference src/lib.rs:176-190; Rust API only): 0, or the mismatch code
 * (101 ksize, 102 DNA/protein, 103 max_hash, 104 seed) with the error slot set. */
int smh_check_compatible(const KmerMinHash *ptr, const KmerMinHash *other);

/* KmerMinHash::intersection (reference src/lib.rs:438-468; the reference header only exports its size):
 * *common_out receives a malloc'ed array (free() it) of the hashes in both sketches that lie inside the
 * bottom-`num` of the union, *n_common their number, *union_size the size of the combined sketch. */
int smh_intersection(const KmerMinHash *ptr, const KmerMinHash *other, uint64_t **common_out, uint64_t *n_common,
                     uint64_t *union_size);

/* The union of partial SCALED sketches without leaving HBM -- what folds the per-GPU partial sketches of one input into one
 * signature (KmerMinHash::merge, reference src/lib.rs:307-403, for scaled sketches: set union, abundances add).
 * smh_sketch_export_dev copies the sketch's ascending hashes (and, when it tracks them and abunds_dev is not NULL, their
 * abundances) into the caller's device buffers of `capacity` entries; *n_out = the number of hashes (call with mins_dev NULL
 * to ask; with a buffer, capacity < *n_out is an error -- Internal -- and nothing is written).  Side effect: a sketch whose
 * state is on the host is MOVED to HBM by the call (its host vectors are emptied; accessors bring it back on demand); a sketch
 * whose abundance vector does not match its hashes (quirks Q5/Q6 after a merge) has no device form and is refused.
 * smh_sketch_absorb_dev unites `ptr` with n_parts sorted, distinct parts lying in ONE device buffer (part k =
 * mins_dev[part_starts[k] .. + part_lens[k]), e.g. the output of an all-gather of padded exports): each part is merged by rank
 * arithmetic and two scatters, no sort, no host copy.  A sketch that tracks abundances needs abunds_dev. */
int smh_sketch_export_dev(KmerMinHash *ptr, uint64_t *mins_dev, uint64_t *abunds_dev, uint64_t capacity, uint64_t *n_out,
                          void *stream);
int smh_sketch_absorb_dev(KmerMinHash *ptr, const uint64_t *mins_dev, const uint64_t *abunds_dev, const uint64_t *part_starts,
                          const uint64_t *part_lens, uint32_t n_parts, void *stream);

/* murmur64 of n byte strings (offsets: n+1 host entries) on the device
 * (reference src/lib.rs:33-35 _hash_murmur) */
int smh_hash_words(const char *bytes, const uint64_t *offsets, uint32_t n, uint64_t seed,
                   uint64_t *out);

/* rows x cols block of compare / intersection_size / count_common / containment between
 * host sketches (reference src/lib.rs:428-436,470-508, src/index.rs:146-154).  Row i is `self`,
 * so its `num` truncates the union walk.  Outputs are row-major n_rows*n_cols, any may be NULL.
 * check_compatible (reference src/lib.rs:176-190) is applied to every pair first. */
int smh_compare_block(KmerMinHash *const *rows, uint32_t n_rows, KmerMinHash *const *cols,
                      uint32_t n_cols, double *jaccard, uint64_t *common, uint64_t *size,
                      uint64_t *count_common, double *containment);

/* The same on device-resident sketches in CSR form: hashes_dev[offsets[i]..offsets[i+1]) is
 * sketch i, ascending and distinct; offsets are HOST arrays.  All sketches share ksize / seed /
 * max_hash / molecule (the caller's index guarantees it); `num` is the rows' num (0 = scaled).
 * Output pointers are device pointers, row-major, any may be NULL. */
int smh_compare_block_dev(const uint64_t *row_hashes_dev, const uint64_t *row_offsets, uint32_t n_rows,
                          const uint64_t *col_hashes_dev, const uint64_t *col_offsets, uint32_t n_cols,
                          uint32_t num, double *jaccard_dev, uint64_t *common_dev, uint64_t *size_dev,
                          uint64_t *count_common_dev, double *containment_dev, void *stream);

/* The all-vs-all matrix of ONE collection resident in HBM, optionally computed by `world` cooperating ranks (one process
 * per GPU) that each hold the whole collection (after an all-gather of the signatures):
 *   1. smh_collection_begin   rank g sorts slice g of hash space (1/world of the pooled hashes: the dictionary pre-pass
 *                             is sharded, not replicated) and leaves its findings in a "share" of smh_collection_share_bytes()
 *                             bytes at smh_collection_share() (device memory, same size on every rank);
 *   2. the caller all-gathers the shares (RCCL; world == 1: nothing to do);
 *   3. smh_collection_finish  assembles the dictionary from the gathered shares (world x share_bytes, rank-major; NULL when
 *                             world == 1): dense ranks of every hash, connected components, frequent hashes, range tables;
 *   4. smh_collection_compare rows [row_lo, row_hi) x ALL columns, outputs row-major (row_hi - row_lo) x n in device memory
 *                             (any may be NULL).  Every pair equals KmerMinHash::compare / count_common of the two sketches
 *                             (reference src/lib.rs:428-436, 470-508) with the one `num` given.  ownership:
 *        0  every pair of the block is computed here;
 *        1  the block is the whole matrix: upper triangle + mirrors (the walk is symmetric when there is one num);
 *        2  the block is this rank's share of a matrix the ranks compute together: row i OWNS the pairs (i, j) with
 *           (j - i) mod n < n/2 (ties: i < j) -- every unordered pair has one owner, every row owns n/2 pairs.  Owned
 *           pairs, pairs whose column is one of the block's own rows, and pairs that share no (non-frequent) hash are
 *           final when the call returns; the others must be taken from their owner's rank, transposed
 *           (sourmash-rust_amd/distributed.py does exactly that with one all-to-all).
 * The dictionary can serve any number of compare calls.  offsets: n+1 HOST entries, sketch i = hashes_dev[offsets[i] ..
 * offsets[i+1]) ascending and distinct; hashes_dev must stay valid until smh_collection_free. */
typedef struct SmhCollection SmhCollection;
SmhCollection *smh_collection_begin(const uint64_t *hashes_dev, const uint64_t *offsets, uint32_t n, uint32_t world,
                                    uint32_t rank, void *stream);
uint64_t smh_collection_share_bytes(const SmhCollection *collection);
const void *smh_collection_share(const SmhCollection *collection);
/* the share copied to dst_dev (e.g. this rank's slot of the all-gather's output buffer) */
int smh_collection_share_to(const SmhCollection *collection, void *dst_dev, void *stream);
int smh_collection_finish(SmhCollection *collection, const void *gathered_dev, void *stream);
int smh_collection_compare(SmhCollection *collection, uint32_t row_lo, uint32_t row_hi, uint32_t num, uint32_t ownership,
                           double *jaccard_dev, uint64_t *common_dev, uint64_t *size_dev, uint64_t *count_common_dev,
                           double *containment_dev, void *stream);
void smh_collection_free(SmhCollection *collection);
/* The exchange that completes ownership 2, device side (8-byte outputs: jaccard, common, size, count_common).
 * smh_mirror_pack: for each of n_blocks peers holding rows [col_lo[b], col_hi[b]), this rank's block out_dev (n_local x
 * n_total) restricted to those columns, TRANSPOSED, packed one block after the other into packed_dev -- the send buffer of
 * an all-to-all.  smh_mirror_apply: from the blocks received (peer b holds rows [peer_lo[b], peer_hi[b]); block b is
 * n_local x (peer_hi[b] - peer_lo[b]) row-major, one after the other in recv_dev) the entries the SENDER's rows own are
 * written into out_dev; row_lo = global index of this rank's first row. */
int smh_mirror_pack(const void *out_dev, uint32_t n_local, uint32_t n_total, const uint32_t *col_lo, const uint32_t *col_hi,
                    uint32_t n_blocks, void *packed_dev, void *stream);
int smh_mirror_apply(void *out_dev, uint32_t row_lo, uint32_t n_local, uint32_t n_total, const uint32_t *peer_lo,
                     const uint32_t *peer_hi, uint32_t n_blocks, const void *recv_dev, void *stream);

/* One query against many nodes: LinearIndex::find (reference src/index/linear.rs:25-45) with
 * search_minhashes / search_minhashes_containment (reference src/index/search.rs:3-9).  Writes the
 * positions of the nodes whose node.similarity(query) -- or node.containment(query) =
 * count_common / |node| (reference src/index.rs:131-161) -- is > threshold, in node order.
 * out_indices must hold n_nodes entries. */
int smh_find(KmerMinHash *const *nodes, uint32_t n_nodes, const KmerMinHash *query, double threshold,
             bool containment, uint32_t *out_indices, uint32_t *out_count);

/* scaffold's nearest leaf (reference src/index/sbt.rs:361-370): position of the candidate with the
 * largest count_common(leaf, candidate) -- the first one on ties, 0 when none is > 0 -- and that
 * count. */
int smh_most_common(const KmerMinHash *leaf, KmerMinHash *const *candidates, uint32_t n,
                    uint32_t *best_pos, uint64_t *best_common);

/* A set of sketches kept resident in HBM (CSR: hashes + offsets + per-node num), so that repeated
 * one-vs-many queries -- LinearIndex::find over a fixed index, reference src/index/linear.rs:25-45 --
 * upload only the query.  Nodes are copied at construction; later changes to them are not seen. */
typedef struct SmhIndex SmhIndex;
SmhIndex *smh_index_new(KmerMinHash *const *nodes, uint32_t n_nodes);
void smh_index_free(SmhIndex *index);
uint32_t smh_index_len(const SmhIndex *index);
/* same contracts as smh_find / smh_most_common, against the resident nodes */
int smh_index_find(SmhIndex *index, const KmerMinHash *query, double threshold, bool containment,
                   uint32_t *out_indices, uint32_t *out_count);
int smh_index_most_common(SmhIndex *index, const KmerMinHash *leaf, uint32_t *best_pos, uint64_t *best_common);
/* rows x cols block between two resident sets (rows' num truncates); host outputs, any may be NULL.  An index compared with
 * ITSELF keeps the dictionary of its collection (dense ranks at 4 B per hash, component roots, the per-sketch partition table
 * of n x (ranges + 1) x 4 B -- ~330 MB for 10 000 long scaled sketches) so that later all-vs-all calls skip the pre-pass;
 * smh_index_drop_dictionary gives that memory back (the next such call rebuilds it), and so does smh_release_workspace()
 * for every live index. */
void smh_index_drop_dictionary(SmhIndex *index);
int smh_index_compare(SmhIndex *rows, SmhIndex *cols, double *jaccard, uint64_t *common, uint64_t *size,
                      uint64_t *count_common, double *containment);

/* Gather: the greedy decomposition of a query against the resident nodes (the min-set-cover loop behind `sourmash gather`;
 * the reference crate has none, so the rules are fixed here -- DESIGN.md 3.9, restated in tests/gather_restatement.py).
 *   Inputs     the n resident sketches S_0 .. S_{n-1}; the query Q, position p = the p-th hash in ascending order;
 *              threshold_common (0 is read as 1); rows_capacity.
 *   Rounds     A_0 = every position of Q.  Round r: c_i = |A_r ^ S_i|; best = the LOWEST i with the largest c_i (the tie
 *              rule of smh_most_common); if c_best < threshold_common or r == rows_capacity the call ends; else
 *              rows[r] = { match = best, common_remaining = c_best, common_original = |Q ^ S_best|, size_match = |S_best|,
 *              abund_sum = sum of the query's abundances over A_r ^ S_best (1 per hash when the query tracks none) },
 *              assigned[p] = r for every p of A_r ^ S_best, and A_{r+1} = A_r \ S_best.
 *   Outputs    *n_rows rows; assigned (nullable, |Q| entries): the round that consumed each position, 0xffffffff for the
 *              positions nobody consumed.  An empty query, an empty index, empty sketches or a query that shares nothing
 *              give zero rows and no error.
 *   Errors     only scaled sketches take part: a query or ANY resident node with num != 0 is SOURMASH_ERROR_CODE_MSG
 *              (decided at this call: such an index still serves smh_index_find); a query that is not compatible with
 *              every node is 101-104 as smh_check_compatible reports it (O(1) when the nodes agree among themselves);
 *              rows == NULL with rows_capacity > 0 is refused.
 * A query whose state lives in HBM (a sketch just built on the device) is read there: nothing is copied to the host.
 * The membership pass over the resident hashes runs once per call; a round is two small launches without host work, and
 * smh_gather_rounds_per_sync() rounds are queued between two read-backs of 8 bytes. */
typedef struct SmhGatherRow {
  uint32_t match, common_remaining, common_original, size_match;
  uint64_t abund_sum;
} SmhGatherRow;   /* 24 bytes */
int smh_index_gather(SmhIndex *index, const KmerMinHash *query, uint32_t threshold_common, SmhGatherRow *rows,
                     uint32_t rows_capacity, uint32_t *n_rows, uint32_t *assigned);
uint32_t smh_gather_rounds_per_sync(void);   /* rounds queued between two read-backs (tests, tools) */

/* Gather of many queries in one call, through the index's hash directory (the directory is the one
 * "Matching records" describes: it is built by the first match or gather-many call on the index and kept).
 *   Equality   For every query q of the batch the rows, their number and `assigned` are exactly what
 *              smh_index_gather(index, queries[q], threshold_common, rows_q, rows_capacity, ...) gives: the tie rule,
 *              threshold_common == 0 read as 1, common_original, size_match, abund_sum (1 per hash for a query without
 *              abundances), and the capacity ending the loop early.  Queries do not interact: the same sketch given twice
 *              gives the same result twice.  No result depends on chunking, budgets or the order of atomics; every output
 *              is an integer, so parity is equality.
 *   Outputs    row_offsets (the caller's, n_queries + 1 entries): the rows of query q are
 *              (*rows)[row_offsets[q] .. row_offsets[q + 1]).  *rows is a malloc'ed array of row_offsets[n_queries] rows
 *              (at least one element is allocated); the caller frees it with free().  query_offsets (nullable,
 *              n_queries + 1 entries): the running sum of the queries' sizes.  assigned (nullable, that sum of entries):
 *              the positions of query q start at query_offsets[q]; 0xffffffff for the positions nobody consumed.
 *   Errors     decided before the device is touched, and nothing is written.  Each query is checked as smh_index_gather
 *              checks it (num != 0 on the query or on any node: SOURMASH_ERROR_CODE_MSG; incompatible: 101-104); when
 *              several queries fail, the error of the LOWEST failing query is reported and the message names that query.
 *              An index of 2^31 or more resident hashes is refused (MSG): the directory takes fewer.  row_offsets == NULL
 *              or rows == NULL is refused.  n_queries == 0, empty queries, an empty index and queries that share nothing
 *              give zero rows and no error.
 * smh_index_gather_many       the queries are sketches.  A query whose state lives in HBM is staged device to device (it is
 *                             not brought to the host); the host-resident queries go up in one upload.
 * smh_index_gather_block_dev  the CSR / device form (next to smh_compare_block_dev): query q is
 *                             q_hashes_dev[q_offsets[q] .. q_offsets[q + 1]), q_offsets on the host (n_queries + 1, ascending),
 *                             q_abunds_dev (nullable: 1 each) one u64 per hash; assigned counts from q_offsets[0].  A CSR
 *                             carries no parameters, so the index's nodes must all be scaled sketches that agree in ksize,
 *                             molecule, seed and max_hash (else MSG).  Hashes must ascend strictly inside a query: the
 *                             caller's contract, as for the compare block.  stream: the caller's.
 * smh_gather_many_set_budget  the (query, node) counters one chunk of the batch may hold: the batch is cut into chunks at
 * smh_gather_many_budget      query boundaries, a query alone always makes a chunk.  0 restores the default of 2^26 -- a memory
 *                             cap, not a measured optimum.  Process-wide; results never depend on it.
 * Per chunk the work is one probe per query hash plus its hits (not a pass over the resident hashes), and one pair of
 * launches serves a round of every query of the chunk; smh_gather_rounds_per_sync() rounds are queued between two
 * read-backs of 8 bytes. */
int smh_index_gather_many(SmhIndex *index, const KmerMinHash *const *queries, uint32_t n_queries, uint32_t threshold_common,
                          uint32_t rows_capacity, uint64_t *row_offsets, SmhGatherRow **rows, uint64_t *query_offsets,
                          uint32_t *assigned);
int smh_index_gather_block_dev(SmhIndex *index, const uint64_t *q_hashes_dev, const uint64_t *q_abunds_dev,
                               const uint64_t *q_offsets, uint32_t n_queries, uint32_t threshold_common, uint32_t rows_capacity,
                               uint64_t *row_offsets, SmhGatherRow **rows, uint32_t *assigned, void *stream);
void smh_gather_many_set_budget(uint64_t pairs);
uint64_t smh_gather_many_budget(void);

/* Search of many queries in one call: the (query, node) pairs over a threshold, as a sparse list (what `manysearch`,
 * `multisearch` and `pairwise` report), through the index's hash directory (the directory is the one
 * "Matching records" describes: it is built by the first match, gather-many, LCA or search-many call on the index and kept).
 * The reference crate has no batch search, so the rules are fixed here; restated in tests/search_many_restatement.py.
 *   Inputs     the n resident sketches S_0 .. S_{n-1}, all scaled (num == 0); a batch of scaled queries Q_0 .. Q_{Q-1};
 *              metric, threshold (double), threshold_common (0 is read as 1).
 *   Per pair   common = |Q_q ^ S_i|, and the metric's value:
 *                SMH_SEARCH_JACCARD            common / max(1, |Q_q| + |S_i| - common)   (smh_index_find's similarity of
 *                                                                                         scaled sketches)
 *                SMH_SEARCH_CONTAINMENT_NODE   common / |S_i|                            (smh_index_find, containment)
 *                SMH_SEARCH_CONTAINMENT_QUERY  common / |Q_q|
 *                SMH_SEARCH_MAX_CONTAINMENT    common / min(|Q_q|, |S_i|)
 *              The value is ONE IEEE binary64 division of the two integers converted to double (the library is built
 *              without fast math).  The pair is reported iff common >= max(1, threshold_common) AND value > threshold:
 *              the comparison is strict, as smh_index_find's.  A pair that shares nothing is never reported, whatever the
 *              threshold is.
 *   Outputs    row_offsets (the caller's, n_queries + 1 entries): the rows of query q are
 *              (*rows)[row_offsets[q] .. row_offsets[q + 1]).  *rows is a malloc'ed array of row_offsets[n_queries]
 *              SmhSearchRow (at least one element is allocated); the caller frees it with free().  The rows are ordered by
 *              query, then by node ascending.  Every field is an integer, so parity is equality; the metric's value, ANI
 *              and the like are derived from the integers by the caller.  No row depends on chunking, the budget or the
 *              order of atomics.
 *   Equality   For threshold >= 0 and threshold_common <= 1 the nodes of query q are exactly, and in the order of,
 *              smh_index_find(index, queries[q], threshold, false, ...) under SMH_SEARCH_JACCARD and
 *              smh_index_find(index, queries[q], threshold, true, ...) under SMH_SEARCH_CONTAINMENT_NODE.
 *   Errors     decided before the device is touched, and nothing is written.  row_offsets == NULL or rows == NULL (a panic, as
 *              every NULL argument), a NaN threshold and an unknown metric (MSG) are refused before anything else is looked at.  Each query is checked
 *              as smh_index_gather_many checks it (num != 0 on the query or on any node: MSG; incompatible: 101-104); the
 *              error of the LOWEST failing query is reported and the message names that query.  An index of 2^31 or more
 *              resident hashes is refused (MSG): the directory takes fewer.  n_queries == 0, empty queries, an empty index
 *              and queries that share nothing give zero rows and no error.  If the rows cannot be allocated the call
 *              returns MSG, having written nothing the caller must free.
 * smh_index_search_many       the queries are sketches.  A query whose state lives in HBM is staged device to device (it is
 *                             not brought to the host); the host-resident queries go up in one upload.
 * smh_index_search_block_dev  the CSR / device form, with the contract of smh_index_gather_block_dev: query q is
 *                             q_hashes_dev[q_offsets[q] .. q_offsets[q + 1]), q_offsets on the host (n_queries + 1,
 *                             ascending); the index's nodes must all be scaled sketches that agree in ksize, molecule, seed
 *                             and max_hash (else MSG); hashes must ascend strictly inside a query.  stream: the caller's.
 * smh_index_search_self       the queries are the index's own nodes, read from the resident CSR in place (no staging copy, no
 *                             upload); row_offsets has smh_index_len(index) + 1 entries.  Rows with node == query are never
 *                             reported; with upper_only only rows with node > query are.  The result equals
 *                             smh_index_search_many of the same sketches with those rows taken out.  Works on an index
 *                             smh_index_downsample returned: its nodes are the cut ones.
 * smh_search_many_set_budget  the (query, node) counters one chunk of the batch may hold: the batch is cut into chunks at
 * smh_search_many_budget      query boundaries, a query alone always makes a chunk.  0 restores the default of 2^26 -- a memory
 *                             cap, not a measured optimum.  Process-wide; results never depend on it.
 * smh_search_geometry         the sizes at which the kernels' branches change: the owners of a hash up to which the lane
 *                             holding the query position walks them itself (longer lists: its wave), the nodes of one
 *                             workgroup of the select and emit kernels, and the most queries a chunk takes (tests, tools).
 * Per chunk the work is one probe per query hash plus one atomic per (position, owner) hit (not a pass over the resident
 * hashes), 4 bytes written and twice 4 bytes read per (query, node) pair, and 16 bytes per reported row. */
enum {
  SMH_SEARCH_JACCARD = 0,
  SMH_SEARCH_CONTAINMENT_NODE = 1,
  SMH_SEARCH_CONTAINMENT_QUERY = 2,
  SMH_SEARCH_MAX_CONTAINMENT = 3
};
typedef struct SmhSearchRow {
  uint32_t node, common, node_size, query_size;
} SmhSearchRow;   /* 16 bytes */
int smh_index_search_many(SmhIndex *index, const KmerMinHash *const *queries, uint32_t n_queries, uint32_t metric, double threshold,
                          uint32_t threshold_common, uint64_t *row_offsets, SmhSearchRow **rows);
int smh_index_search_block_dev(SmhIndex *index, const uint64_t *q_hashes_dev, const uint64_t *q_offsets, uint32_t n_queries,
                               uint32_t metric, double threshold, uint32_t threshold_common, uint64_t *row_offsets,
                               SmhSearchRow **rows, void *stream);
int smh_index_search_self(SmhIndex *index, uint32_t metric, double threshold, uint32_t threshold_common, bool upper_only,
                          uint64_t *row_offsets, SmhSearchRow **rows);
void smh_search_many_set_budget(uint64_t pairs);
uint64_t smh_search_many_budget(void);
void smh_search_geometry(uint32_t *short_owners, uint32_t *node_tile, uint32_t *max_queries);

/* Nearest neighbours: per query the best k nodes, best first -- a bounded, ordered result that needs no guessed threshold
 * (`search --best-only`, `--num-results N`, classifying by the closest reference, the k-nearest-neighbour graph of a
 * collection).  The reference crate has no such call, so the rules are fixed here; restated in
 * tests/nearest_restatement.py.
 *   Rows of q  the rows smh_index_search_many reports for query q under the same metric, threshold and threshold_common: the
 *              same rule, through the same device function -- the comparison is strict, common >= max(1, threshold_common),
 *              and a pair that shares nothing is never a neighbour, whatever the threshold is (a threshold below 0 keeps
 *              every pair that shares a hash).
 *   Order      by value DESCENDING, where the value is the ONE IEEE binary64 division that "Per pair" above defines for the
 *              metric; then by node ASCENDING among rows whose values are equal AS DOUBLES.  Two different fractions that
 *              round to the same double (1/2 and 2/4 always do; so may two near-equal fractions of large integers) are a
 *              tie, and the node decides it.  The value is positive, so its bit pattern read as an unsigned 64-bit integer
 *              is its order: the device sorts by the key (value bits, ~node), descending.
 *   Result     the first min(k, rows) rows of that order.
 *   Outputs    row_offsets (the caller's, n_queries + 1 entries) and *rows, a malloc'ed array of row_offsets[n_queries]
 *              SmhSearchRow (at least one element is allocated; the caller frees it with free()): the struct, and the integers
 *              in it, are exactly what smh_index_search_many returns for the pair.  The rows of a query are in the order
 *              above (NOT by node).  No row depends on chunking, the budget (smh_search_many_set_budget governs the chunks
 *              here too), the grid or the order of atomics: a node appears once per query, so no two keys are equal.
 *   Errors     decided before the device is touched, and nothing is written: everything smh_index_search_many refuses, in the
 *              same order; behind the NaN threshold and the unknown metric, k == 0 and k > max_k (MSG; the message names
 *              the limit, which smh_nearest_geometry reports).
 * smh_index_nearest_many       the queries are sketches, staged as smh_index_search_many stages them.
 * smh_index_nearest_block_dev  the CSR / device form, with the contract of smh_index_search_block_dev.
 * smh_index_nearest_self       the k-nearest-neighbour graph: the queries are the index's own nodes, read from the resident CSR
 *                              in place; row_offsets has smh_index_len(index) + 1 entries.  node == query is never reported
 *                              (and takes none of the k places).  Works on an index smh_index_downsample returned.
 * smh_nearest_geometry         the sizes at which the kernels' branches change: the largest k (256), the nodes of one workgroup
 *                              of the tile kernel (smh_search_geometry's), and the keys the merge sorts at once -- a query
 *                              whose kept candidates exceed merge_slots - k takes more than one merge step (tests, tools).
 * Per chunk the work is smh_index_search_many's up to the select; then, instead of 16 bytes per surviving pair, a sort in LDS
 * of every tile that holds a survivor, 12 bytes of work space per kept candidate (at most k per tile), and 16 bytes per
 * reported row, at most k per query. */
int smh_index_nearest_many(SmhIndex *index, const KmerMinHash *const *queries, uint32_t n_queries, uint32_t k, uint32_t metric,
                           double threshold, uint32_t threshold_common, uint64_t *row_offsets, SmhSearchRow **rows);
int smh_index_nearest_block_dev(SmhIndex *index, const uint64_t *q_hashes_dev, const uint64_t *q_offsets, uint32_t n_queries,
                                uint32_t k, uint32_t metric, double threshold, uint32_t threshold_common, uint64_t *row_offsets,
                                SmhSearchRow **rows, void *stream);
int smh_index_nearest_self(SmhIndex *index, uint32_t k, uint32_t metric, double threshold, uint32_t threshold_common,
                           uint64_t *row_offsets, SmhSearchRow **rows);
void smh_nearest_geometry(uint32_t *max_k, uint32_t *node_tile, uint32_t *merge_slots);

/* Clustering a resident index: the pairs of smh_index_search_self stay on the device and come back as clusters, 8 bytes per
 * node.  The reference crate has no clustering, so the rules are fixed here; restated in
 * tests/cluster_restatement.py.
 *   Inputs     the n resident sketches, all scaled (num == 0); a metric, threshold (double), threshold_common (0 is read as 1),
 *              a linkage, and scores (n entries; NULL: score[v] = |S_v|).
 *   Adjacency  u ~ v (u != v) iff the pair survives smh_index_search_self's rule -- the kernels call the same device function:
 *              common >= max(1, threshold_common) AND one IEEE binary64 division > threshold, strictly.  Only the symmetric
 *              metrics are taken, SMH_SEARCH_JACCARD and SMH_SEARCH_MAX_CONTAINMENT; the two directed containments are
 *              refused (MSG): either direction exceeding a threshold is what max-containment says.
 *   Priority   v comes before u iff score[v] > score[u], or the scores are equal and v < u.
 *   SMH_CLUSTER_COMPONENTS  single linkage: the clusters are the connected components of ~; a cluster's representative is its
 *              member first in priority.
 *   SMH_CLUSTER_GREEDY      walk the nodes in priority order: v becomes a representative iff no earlier representative is
 *              adjacent to it.  When the representatives are final, every other node joins the adjacent representative with
 *              the greatest value (the rule's own double); ties go to the representative earlier in priority -- which may come
 *              later than v in priority.  It does not chain.
 *   Outputs    the caller's arrays of n entries: cluster[v] (clusters are numbered 0, 1, ... in ascending order of their
 *              smallest member node), representative[v] (a node), rep_common[v] (nullable; GREEDY only: |S_v ^ S_rep| for a
 *              member, |S_v| for a representative), and *n_clusters.  Every output is an integer, so parity is equality; none
 *              depends on chunking, on any budget, on smh_cluster_rounds or on the order of atomics.  A node adjacent to
 *              nothing (an empty sketch included) is its own cluster; n == 0 gives *n_clusters = 0.
 *   Errors     decided before the device is touched, and nothing is written.  cluster, representative or n_clusters NULL: a
 *              panic, as every NULL argument.  A NaN threshold, an unknown or directed metric, an unknown linkage, rep_common
 *              with COMPONENTS: MSG.  A num sketch in the index: MSG.  Nodes that refuse each other and an index of 2^31 or
 *              more hashes: as smh_index_search_self.
 *   Budgets    The (query, node) counters are cut into chunks as smh_index_search_self's, under smh_search_many_set_budget.
 *              GREEDY keeps the directed adjacency in device memory (8 bytes per entry; 16 while a chunk is collected): when
 *              the entries exceed smh_cluster_pair_budget() the call fails with MSG -- the message names the count reached
 *              and the budget -- as soon as a chunk's running total passes it, and nothing is written.  COMPONENTS holds
 *              nothing proportional to the pairs.
 * smh_cluster_set_pair_budget  0 restores the default of 2^27 directed entries -- a memory cap, not a measured optimum.
 * smh_cluster_set_rounds       the greedy rounds queued between two 8-byte read-backs of the undecided count; 0 restores the
 *                              default of 32 (smh_gather_rounds_per_sync's choice).  Results never depend on it.
 * smh_cluster_geometry         lane_max: the adjacency-list length up to which one lane walks a node's list in a greedy round
 *                              and in the assignment (longer lists: its wave); node_tile: the nodes of one workgroup of the
 *                              linking pass (tests, tools).
 * smh_index_sizes              sizes[v] = |S_v| of every node as the index holds it (n entries; host only, no device work):
 *                              what turns rep_common into the metric's value on the caller's side.
 * Works on an index smh_index_downsample returned: its nodes are the cut ones. */
enum {
  SMH_CLUSTER_COMPONENTS = 0,
  SMH_CLUSTER_GREEDY = 1
};
int smh_index_cluster(SmhIndex *index, uint32_t metric, double threshold, uint32_t threshold_common, uint32_t linkage,
                      const uint32_t *scores, uint32_t *cluster, uint32_t *representative, uint32_t *rep_common,
                      uint32_t *n_clusters);
void smh_cluster_set_pair_budget(uint64_t entries);
uint64_t smh_cluster_pair_budget(void);
void smh_cluster_set_rounds(uint32_t rounds);
uint32_t smh_cluster_rounds(void);
void smh_cluster_geometry(uint32_t *lane_max, uint32_t *node_tile);
int smh_index_sizes(const SmhIndex *index, uint32_t *sizes);

/* Collapsing an index by groups: one sketch per group of nodes -- the union (`sig merge`), the core (`sig intersect`), the
 * hashes at least x % of the members hold, or the hash -> number-of-members table -- made on the device from the index's
 * hash directory, as a new resident index.  The reference crate has no counterpart, so the rules are fixed
 * here; restated in tests/collapse_restatement.py.
 *   Inputs     an index of n nodes; n_groups = G; group[v] for every node, each < G or SMH_COLLAPSE_DROP (the node takes no
 *              part); min_count; min_fraction (double); an abundance mode.
 *   m_g        the number of nodes with group[v] == g.
 *   c_g(h)     the number of those nodes that hold hash h;  a_g(h): the exact unsigned 64-bit sum of their abundances of h.
 *   need_g     max(1, min_count, ceil(min_fraction * m_g)).  The product and the ceiling are taken in IEEE binary64 on the
 *              host (Python: math.ceil(min_fraction * m)); the device sees the G integers only.
 *   Result     an index of G sketches; sketch g = { h : c_g(h) >= need_g }, ascending as unsigned 64-bit.  min_count = 1 and
 *              min_fraction = 0 give the union, min_fraction = 1.0 the intersection.  A group with m_g == 0 or need_g > m_g is
 *              an empty sketch; n == 0 gives G empty sketches.
 *   SMH_COLLAPSE_FLAT   no abundances: smh_index_has_abundances is false for the result.
 *   SMH_COLLAPSE_SUM    the abundance of h in sketch g is a_g(h).
 *   SMH_COLLAPSE_COUNT  the abundance of h in sketch g is c_g(h), the prevalence table; it cannot overflow.
 *   Parameters the result's nodes take node 0's ksize, molecule, seed and max_hash, and are scaled sketches; abundances are
 *              tracked exactly when the mode is not FLAT.  (An index without nodes has no parameters to hand down: DNA,
 *              ksize 21, seed 42, max_hash 2^64 - 1.)  The result carries NO taxonomy -- its nodes are not the parent's -- keeps
 *              no reference to the parent, and is an index like any other: every call here takes it, this one included.
 *   Refused    with SOURMASH_ERROR_CODE_MSG, the message names the offending entry, NULL is returned, and nothing is built:
 *              G == 0; min_fraction outside [0, 1] or NaN; an unknown mode (these three before the index or the device is
 *              looked at); index NULL, or group NULL for an index with nodes; a node that is not a scaled sketch
 *              (smh_index_all_scaled); nodes that do not agree in ksize, molecule, seed and max_hash (smh_index_downsample
 *              brings them to one max_hash); a group[v] >= G that is not SMH_COLLAPSE_DROP; SUM on an index for which
 *              smh_index_has_abundances is false or that holds an abundance of 2^32 or more (worded as the angular calls
 *              word it); an index of 2^31 or more hashes (the directory's own refusal); SUM where a KEPT sum is 2^32 or
 *              more -- the message names the lowest such group.  Only that last refusal is found on the device (one
 *              atomicMin on an error word); the work space of the call is back in the pool when it returns.
 *   Device     the hash directory (built by the first call that needs it and kept, counter "match_directory_built") is read
 *              twice, by a count pass and an emit pass; the survivors -- (group, rank of the hash) pairs -- are partitioned by
 *              group with a stable sort on the group's bytes, the groups' bounds are searched among the sorted keys, and
 *              4 G + 8 bytes come to the host.  SUM first moves the
 *              abundances to HBM as the first angular call does.  Work space, all from the block pool and all returned: 4 B
 *              per distinct hash of the index, 16 B per survivor (24 B with abundances) while they are partitioned, 8 G B,
 *              4 B per node, and the lists of the long owner lists (at most 4 B per 9 resident hashes).  There is no
 *              chunking: a call that does not fit fails with the pool's own error.  Inside one hash the survivors are
 *              written in no fixed order -- a group appears once per hash, so the partition yields the same bytes.
 * smh_collapse_geometry  lane_max: the owner-list length up to which one lane folds a hash's owners; wave_max: up to which
 *                        one wave does, the owners' groups in its LDS scratch; group_tile: the groups one round of LDS
 *                        counters covers for a longer list (tests, tools).
 * smh_index_read         the index as it is held: offsets (n + 1 entries, from 0), hashes and abunds (offsets[n] entries
 *                        each; the caller sizes them from smh_index_sizes).  Each of the three may be NULL.  The hashes
 *                        come from the device CSR, the abundances from the host copy or from HBM, wherever they live.
 *                        abunds asked of an index for which smh_index_has_abundances is false, or that holds an abundance
 *                        of 2^32 or more: MSG, nothing written.  Works on every index: built from sketches, downsampled,
 *                        collapsed.
 * Timers under smh_profile_get: "collapse_count", "collapse_emit", "collapse_partition", "collapse_finish"; event counter:
 * "index_collapsed". */
enum {
  SMH_COLLAPSE_FLAT = 0,
  SMH_COLLAPSE_SUM = 1,
  SMH_COLLAPSE_COUNT = 2
};
#define SMH_COLLAPSE_DROP 0xffffffffu
SmhIndex *smh_index_collapse(SmhIndex *index, const uint32_t *group, uint32_t n_groups, uint32_t min_count, double min_fraction,
                             uint32_t abund);
void smh_collapse_geometry(uint32_t *lane_max, uint32_t *wave_max, uint32_t *group_tile);
int smh_index_read(SmhIndex *index, uint64_t *offsets, uint64_t *hashes, uint32_t *abunds);

/* Building an index from records: the records of a batch hashed, folded by group and laid out as a resident index without
 * leaving the device -- one group of records, one node -- and the concatenation of resident indexes in HBM.
 * The reference crate has no counterpart, so the rules are fixed here; restated in tests/index_build_restatement.py.  They
 * are all integers: results are EQUAL, never close.
 *   like       gives the parameters only: ksize, molecule, seed, max_hash and whether abundances are tracked.  Its contents
 *              are not read and it is not modified.  It must be a scaled sketch (num == 0, max_hash != 0).
 *   Groups     groups[r] < n_groups says which node record r feeds.  groups == NULL: record r is node r, and n_groups must
 *              equal n_records (no group ids are uploaded then).  A group with no records, or whose records yield no
 *              sampled hash, is an empty node; n_groups == 0 gives an index of 0 nodes.
 *   SMH_INPUT_NUCLEOTIDE on a DNA `like`: node g holds exactly what smh_add_sequences_grouped(..., force = true) leaves in
 *              a FRESH sketch of like's parameters for group g -- the hashes <= max_hash of every window of ksize bases of
 *              the group's records, ascending and distinct; with abundances, each hash carries the number of windows of
 *              the group's records that have it, as u32.  There is no `force` argument: windows holding a byte outside
 *              ACGTacgt are skipped, as smh_index_match_* skips them.  On a protein / dayhoff / hp `like` it is the
 *              translated six-frame arm of smh_add_sequences_grouped, with its errors (the UTF-8 panic of a byte >= 0x80).
 *   SMH_INPUT_AMINO  smh_add_proteins per group: every window of ksize / 3 residues.  It needs a protein, dayhoff or hp
 *              `like`; a DNA one is refused as smh_add_protein refuses it.
 *   Result     every node gets like's parameters: the index is uniform and all-scaled (smh_index_all_scaled), so match,
 *              lca, collapse and cluster take it as it is; smh_index_has_abundances is like's flag.  It carries no taxonomy,
 *              no dictionary and no directory; they are built on first use like any index's.
 *   Refused    with SOURMASH_ERROR_CODE_MSG, NULL is returned and no half-built index stays registered.  Before the device
 *              is touched and with nothing written: like, offsets or seq NULL; an unknown `input`; a bottom-num `like`;
 *              SMH_INPUT_AMINO with a DNA `like`; offsets that do not ascend or reach beyond the batch; groups[r] >=
 *              n_groups (the message names r); groups == NULL with n_groups != n_records; a window size of 0 (ksize == 0,
 *              or ksize / 3 == 0 off DNA: where the grouped path panics); n_groups >= 2^24 (the grouped fold tags a
 *              candidate with its group in 24 bits; smh_index_concat joins the pieces).  After hashing: with abundances,
 *              a (group, hash) seen in 2^32 or more windows -- the message names the lowest such group, worded as
 *              smh_index_collapse words its SUM refusal; more than 2^31 - 1 (group, hash) pairs in the result.
 *   Budget     smh_index_build_set_budget(candidates) bounds the work space: a fold is a stretch of the batch's position
 *              space expected to leave that many candidates -- positions x (max_hash + 1) / 2^64, the notion of
 *              smh_match_set_pair_budget -- cut where the grouped path cuts its chunks, inside records too.  A hash of one
 *              group that shows up in several folds is one hash with the counts added.  THE RESULT NEVER DEPENDS ON IT.
 *              0 restores the default, 2^26: a memory cap chosen by reasoning (about 4 GiB: 40 B of sort buffers per
 *              candidate with their head-room, 20 B per run), not a tuned figure.
 *   Device     per fold the hashing kernel of the arm, positions -> groups, the sort by hash and the stable sort by group,
 *              as the grouped path runs them; then, instead of its read-back, a head count over tiles of tile_elems
 *              candidates, a scan, an ordered emit (ballot / popcount, no cursor) and the runs' counts.  The runs of several
 *              folds are merged by one more sort by (group, hash) and the same kernels with the counts as weights.  One
 *              bisecting lane per group finds the offsets.  Per fold the candidate count and the run count come to the
 *              host, per call the 8 (n_groups + 1) bytes of offsets; nothing proportional to the hashes crosses in
 *              either direction.  Work space comes from the block pool and is back there when the call returns.
 * smh_index_concat  a new index whose nodes are those of parts[0], then parts[1], and so on.  Parts may be any resident
 *              indexes -- built from sketches, cut, collapsed, built here; scaled or num; of mixed parameters.  Hashes
 *              are copied device to device, abundances from wherever each part keeps them (host copy or HBM); offsets are
 *              rebased; parameters and nums are copied and what is decided once per index is decided again.  Abundances
 *              are kept exactly when every part has them.  The result owns its memory -- the parts may be freed -- and
 *              carries no taxonomy, dictionary or directory (merging built directories is not done).  Refused (MSG):
 *              parts NULL with n_parts > 0, a NULL part, more than 2^32 - 2 nodes in all.  n_parts == 0: an empty index.
 * smh_index_build_geometry  tile_elems: the candidates one workgroup of the head and emit passes takes; threads: its size.
 * Timers under smh_profile_get: "index_build_heads", "index_build_emit", "index_build_merge"; event counters:
 * "index_build_fold", "index_built", "index_concat". */
enum {
  SMH_INPUT_NUCLEOTIDE = 0,
  SMH_INPUT_AMINO = 1
};
SmhIndex *smh_index_from_sequences(const KmerMinHash *like, int input, const char *seq, const uint64_t *offsets,
                                   const uint32_t *groups, uint32_t n_records, uint32_t n_groups);
SmhIndex *smh_index_from_sequences_dev(const KmerMinHash *like, int input, const void *seq_dev, uint64_t total_len,
                                       const uint64_t *offsets, const uint32_t *groups, uint32_t n_records,
                                       uint32_t n_groups, void *stream);
SmhIndex *smh_index_from_records(const KmerMinHash *like, int input, const SmhRecords *r, const uint32_t *groups,
                                 uint32_t n_groups);
SmhIndex *smh_index_concat(SmhIndex *const *parts, uint32_t n_parts);
void smh_index_build_set_budget(uint64_t candidates);
uint64_t smh_index_build_budget(void);
void smh_index_build_geometry(uint32_t *tile_elems, uint32_t *threads);

/* Filtering an index: a new resident index that holds a subset of each node of its parent -- `sig subtract`, `sig intersect`
 * against a mask, `sig inflate`, `sig filter` (an abundance window), `sig flatten`, the hashes held by exactly one / at most x
 * / at least x nodes -- and a new index that holds a subset of the parent's nodes, both made on the device.
 * The reference crate has no counterpart, so the rules are fixed here; restated in tests/filter_restatement.py.  They are all
 * integers: results are EQUAL, never close.
 * smh_index_filter  The child has the parent's n nodes, in order, with the parent's parameters.  Node i of the child holds,
 *              ascending, the hashes h of parent node i for which ALL three conditions hold.  Each condition is evaluated on
 *              the PARENT: the conditions do not see each other's effect.
 *   Operand    SMH_FILTER_KEEP_IN: h is in the operand.  SMH_FILTER_DROP_IN: h is not in the operand.
 *              SMH_FILTER_OPERAND_NONE: always true; the operand may then be NULL and is not looked at.
 *   Abundance  min_abund <= a <= max_abund, a the node's own abundance of h.  0, 0xffffffff: no window.
 *   Owners     min_owners <= owners(h) <= max_owners, owners(h) the number of parent nodes that hold h: the length of h's
 *              owner list in the hash directory.  min_owners 0 or 1 with max_owners 0xffffffff: no window.  max_owners = 1
 *              gives every node its private hashes, min_owners = 2 the shared ones.  The directory is built (counter
 *              "match_directory_built") ONLY when this window is not trivial and the index holds a hash.
 *   Abundances of the child.  SMH_FILTER_ABUND_OWN: the parent's, for the kept hashes; the child has abundances iff the parent
 *              has.  SMH_FILTER_ABUND_FLAT: none.  SMH_FILTER_ABUND_OPERAND: the operand's abundance of h (`sig inflate`); it
 *              needs KEEP_IN and an operand that tracks abundances.
 *   Result     carries the parent's taxonomy (same nodes, same order), no compare dictionary and no hash directory of its
 *              own; its abundances, when it has them, are resident in HBM.  It is an index like any other.
 *   Refused    with SOURMASH_ERROR_CODE_MSG and a message that begins with "filter:" -- except an operand incompatible with
 *              the nodes, which is 101-104 as smh_check_compatible reports them -- NULL is returned, and every refusal is
 *              decided before anything is built: rule NULL; an unknown operand_mode or abund_out; min > max in either
 *              window; OPERAND without KEEP_IN (these before the index or the device is looked at); index NULL; a node that
 *              is not a scaled sketch; operand NULL when operand_mode is not NONE; an operand that is not a scaled sketch;
 *              OPERAND with an operand that tracks no abundances; an abundance window on an index for which
 *              smh_index_has_abundances is false; abundances involved (an abundance window, or OWN on an index with
 *              abundances) and a node holding an abundance of 2^32 or more -- the message names the node; OPERAND with an
 *              operand abundance of 2^32 or more, or whose abundance vector does not match its hashes; an owner window on
 *              an index of 2^31 or more hashes (the directory's own refusal); an operand of 2^31 or more hashes.
 *   Empty      an empty index, empty nodes, an empty operand, a rule that keeps nothing: zero-length nodes, no error.
 *   Device     an operand whose state lives in HBM is read there ("sketch_to_host" does not move), a host operand goes up in
 *              one upload.  Parent abundances still on the host are uploaded for the call, those in HBM are read in place.
 *              A flag pass gives every resident hash its verdict -- the operand and the directory are searched per hash,
 *              their sampled tops in LDS -- as one bit, and counts the survivors per tile of `tile` hashes; the counts are
 *              scanned 64 bits wide (an index promises no total below 2^32); one lane per node finds its new offset; an emit
 *              pass writes the survivors in order.  Under OPERAND the emit pass searches the operand again for the survivors
 *              (no position is stored per hash).  8 (n + 1) bytes of offsets come to the host; nothing proportional to the
 *              hashes does.  Work space, from the block pool and returned: 256 B of mask per tile (one bit per hash, rounded
 *              up to whole tiles) and 8 B per tile + 8; 4 B per hash more when the parent's abundances are uploaded.
 * smh_index_select  Node j of the child is node ids[j] of the parent, whole: any order, repeats allowed, n_ids may be 0.  It
 *              works on ANY index, num sketches included: it only copies, device to device.  Carried: the per-node
 *              parameters and nums, the abundances wherever the parent has them (host or HBM), the taxonomy (the same
 *              parents, the nodes' taxa permuted).  Refused (MSG, "select:"): index NULL; ids NULL with n_ids > 0; an
 *              id >= n -- the message names its position.
 * smh_filter_geometry  tile: the hashes one workgroup trip of the flag and emit passes takes; operand_samples: the sampled
 *              top of the operand the search keeps in LDS (an operand up to that size is searched in LDS alone); threads:
 *              the workgroup's size (tests, tools).
 * Timers under smh_profile_get: "filter_flag", "filter_emit"; event counters: "index_filtered", "index_selected". */
enum { SMH_FILTER_OPERAND_NONE = 0, SMH_FILTER_KEEP_IN = 1, SMH_FILTER_DROP_IN = 2 };
enum { SMH_FILTER_ABUND_OWN = 0, SMH_FILTER_ABUND_FLAT = 1, SMH_FILTER_ABUND_OPERAND = 2 };
typedef struct SmhFilter {
  uint32_t operand_mode, abund_out;
  uint32_t min_abund, max_abund;     /* 0, 0xffffffff: no window */
  uint32_t min_owners, max_owners;   /* 0 or 1, 0xffffffff: no window */
} SmhFilter;
SmhIndex *smh_index_filter(SmhIndex *index, const KmerMinHash *operand, const SmhFilter *rule);
SmhIndex *smh_index_select(SmhIndex *index, const uint32_t *ids, uint32_t n_ids);
void smh_filter_geometry(uint32_t *tile, uint32_t *operand_samples, uint32_t *threads);

/* Angular similarity on abundances: what `sourmash compare` and `sourmash search` report by default for sketches that
 * track abundances.  The reference crate has no weighted compare, so the rules are fixed here -- DESIGN.md 3.10, restated
 * in tests/angular_restatement.py.  For two sketches A and B that both track abundances, hashes ascending and distinct, one
 * abundance per hash:
 *   norm2(A)   the sum of a_h^2 over the hashes h of A.
 *   dot(A, B)  the sum of a_h * b_h over the hashes h that A and B both hold.
 *   Exactness  both are exact unsigned 64-bit integers.  A sketch whose norm2 does not fit 64 bits is refused with
 *              SOURMASH_ERROR_CODE_MSG and the message names the node (the LOWEST one when several are bad); that includes
 *              any single abundance of 2^32 or more.  So every accepted abundance fits 32 bits, and since
 *              dot <= sqrt(norm2(A) * norm2(B)) <= max(norm2), the dot of two accepted sketches cannot overflow.
 *   cosine     as double, in exactly this order: c = (double)dot / (sqrt((double)norm2A) * sqrt((double)norm2B)); every
 *              conversion rounds to nearest; IEEE sqrt, multiply and divide (no fast math, no reciprocal).  dot == 0 or a
 *              norm of 0: c = 0.0.  c > 1.0: c = 1.0.  (For a sketch against itself the literal formula can land one or
 *              two ulp below 1.0 -- sqrt(n) * sqrt(n) need not round back to n -- so the matrix of an index with ITSELF
 *              sets its diagonal, see smh_index_angular.)
 *   angular    as double: 0.0 when c == 0.0, 1.0 when c == 1.0, else 1.0 - (2.0 * acos(c)) / M_PI.
 *   num        does not truncate: every hash of both sketches takes part, as in sourmash.
 *   Compatible check_compatible applies to every pair: 101-104 as smh_check_compatible reports them.
 *   Refused    with SOURMASH_ERROR_CODE_MSG: a sketch that does not track abundances; a sketch whose abundance vector does
 *              not match its hashes (quirks Q5/Q6 after a merge; smh_sketch_export_dev refuses the same case).
 *   Empty      sketches are no error: dot = 0, cosine = 0.0, angular = 0.0.
 * Argument and parameter checks come before the device is touched.
 *
 * smh_index_has_abundances  true when EVERY node tracked abundances, with a vector that matched its hashes, when the index
 *                           was built.  Such an index keeps the abundances narrowed to 32 bits on the host (a copy, like the
 *                           hashes); the first angular call moves them to HBM (4 B per hash) and computes the norms.  find,
 *                           compare and gather on the index are unchanged, and an index nobody asks pays no HBM.
 * smh_index_norms2          norm2 of every node, n entries.
 * smh_index_angular         rows x cols, host outputs, row-major, any may be NULL.  rows == cols: only col > row is walked and
 *                           mirrored (the matrix equals its transpose bit for bit) and the diagonal is dot = norm2, cosine =
 *                           angular = 1.0 (0.0 for an empty sketch).  From smh_angular_prune_min_pairs() pairs on, the block
 *                           compare first computes count_common (for an index against itself through its cached dictionary,
 *                           see smh_index_compare) and only the pairs that share a hash are walked.  Device memory, all
 *                           from the block pool: 8 B per pair and requested output, plus 8 B per pair when pruning.
 * smh_index_angular_query   one query against every node: dot / cosine / angular with n entries each, query_norm2 with n
 *                           entries all holding the query's norm2 (any may be NULL).  A query whose state lives in HBM is
 *                           read there, as gather reads it.
 * smh_angular_similarity    one pair through the same kernel; any output may be NULL.
 * smh_angular_block_dev     the CSR / device form, next to smh_compare_block_dev: hashes (u64) and abundances (u32) in device
 *                           memory, offsets (n + 1 entries) on the host; outputs stay on the device (any may be NULL;
 *                           row_norm2_dev / col_norm2_dev receive n_rows / n_cols entries).  count_common_dev (nullable):
 *                           a row-major u64 matrix, a pair whose entry is 0 is not walked and gets the zero outputs.
 *                           symmetric: rows and columns are the same sketches, handled as rows == cols above.
 * smh_angular_last_stats    of the last angular call: pairs whose column was streamed against the row, and pairs that got
 *                           the zero outputs without a walk (pruned, or one side empty).  The diagonal and the mirrored
 *                           half of a symmetric block are in neither.
 * smh_angular_set_prune_min_pairs  process-wide; 0 restores the default, UINT64_MAX never prunes, 1 always does.  The result
 *                           never depends on it. */
bool smh_index_has_abundances(const SmhIndex *index);
int smh_index_norms2(SmhIndex *index, uint64_t *out);
int smh_index_angular(SmhIndex *rows, SmhIndex *cols, uint64_t *dot, double *cosine, double *angular);
int smh_index_angular_query(SmhIndex *index, const KmerMinHash *query, uint64_t *dot, uint64_t *query_norm2, double *cosine,
                            double *angular);
int smh_angular_similarity(const KmerMinHash *a, const KmerMinHash *b, double *angular, double *cosine, uint64_t *dot,
                           uint64_t *norm2_a, uint64_t *norm2_b);
int smh_angular_block_dev(const uint64_t *row_hashes_dev, const uint32_t *row_abunds_dev, const uint64_t *row_offsets,
                          uint32_t n_rows, const uint64_t *col_hashes_dev, const uint32_t *col_abunds_dev,
                          const uint64_t *col_offsets, uint32_t n_cols, const uint64_t *count_common_dev, bool symmetric,
                          uint64_t *dot_dev, uint64_t *row_norm2_dev, uint64_t *col_norm2_dev, double *cosine_dev,
                          double *angular_dev, void *stream);
void smh_angular_last_stats(uint64_t *pairs_walked, uint64_t *pairs_skipped);
uint64_t smh_angular_prune_min_pairs(void);
void smh_angular_set_prune_min_pairs(uint64_t pairs);

/* Downsampling: cutting scaled sketches and resident indexes at a coarser resolution, so that operands sketched at
 * different `scaled` can meet (every search route refuses operands whose max_hash differ, 103).  The reference crate has
 * no downsampling, so the rules are fixed here -- DESIGN.md 3.12, restated in tests/downsample_restatement.py.
 *   Scaled sketch   num == 0 and max_hash != 0 (the test gather applies).
 *   max_hash cut    keeps the hashes h <= new max_hash (unsigned, inclusive: the comparison add_hash makes) and their
 *                   abundances when tracked; every other parameter is kept; the result has max_hash = new.  A scaled sketch
 *                   is the ascending set of its hashes <= max_hash, so the cut is an exact prefix: nothing is hashed again.
 *                   new == max_hash gives an equal, independent copy.
 *   Refused         with SOURMASH_ERROR_CODE_MSG and a message naming the values: new == 0; new > max_hash (a sketch cannot
 *                   be made finer); a sketch that is not a scaled sketch.
 *   num cut         keeps the first `num` hashes (and abundances) of a sketch with num != 0 and max_hash == 0; the result has
 *                   num = new.  Refused (MSG) for new == 0, new > num, and a sketch with max_hash != 0.  Host only.
 *   Meeting         two scaled operands that differ in max_hash meet at the smaller of the two; ksize, seed and molecule
 *                   still have to agree and raise what they raise today.
 * The ABI speaks max_hash only (max_hash = min(2^64 / scaled, 2^64 - 1)).
 *
 * smh_kmerminhash_downsample_max_hash  a new sketch.  A host-resident sketch is cut on the host (no device needed).  A sketch
 *                           whose state lives in HBM is cut there: the bound is found by a kernel, the prefixes of its arrays
 *                           are copied device to device into a state of the new sketch's own, and 16 bytes come back (the
 *                           cut and the new total).  Neither sketch is brought to the host.  NULL on failure.
 * smh_kmerminhash_downsample_num       a new sketch, cut on the host.  NULL on failure.
 * smh_index_downsample      a new, owned index holding the parent's nodes cut at max_hash, in the parent's order, built from
 *                           the parent's device arrays: a bounds pass (one wave per node), the kept lengths to the host
 *                           (4 B per node), then a copy balanced over the output.  Refused (MSG) when a node is not a
 *                           scaled sketch, when max_hash is 0, and when it exceeds the smallest max_hash of a node.  A parent
 *                           whose nodes differ in max_hash is thereby brought to one resolution.  The child has abundances
 *                           exactly when the parent has, keeps no reference to the parent and builds its own dictionary.
 *                           An abundance of 2^32 or more (see the angular rules) counts only at a position the cut kept.
 *                           NULL on failure.
 * smh_index_max_hash_range  the smallest and the largest max_hash over the nodes; 0, 0 for an empty index.
 * smh_index_all_scaled      true when every node was a scaled sketch when the index was built (also for an empty index):
 *                           what smh_index_downsample requires.  Decided once, at construction.
 * smh_downsample_block_dev  the CSR / device form, next to smh_compare_block_dev: hashes (u64) and optional abundances (u32)
 *                           in device memory, offsets (n + 1) on the host.  The kept prefixes are written densely to
 *                           out_hashes_dev / out_abunds_dev, out_offsets (host, n + 1 entries) start at 0.  capacity counts
 *                           elements: when the kept total exceeds it the call fails with MSG before it writes anything (a
 *                           capacity equal to the input total always suffices).  Outputs must not alias inputs.
 * smh_downsample_geometry   output elements per workgroup of the copy, and its threads (tests, tools).
 * Timers under smh_profile_get: "downsample_bounds", "downsample_copy"; event counter: "index_downsampled". */
KmerMinHash *smh_kmerminhash_downsample_max_hash(const KmerMinHash *ptr, uint64_t max_hash);
KmerMinHash *smh_kmerminhash_downsample_num(const KmerMinHash *ptr, uint32_t num);
SmhIndex *smh_index_downsample(SmhIndex *index, uint64_t max_hash);
int smh_index_max_hash_range(const SmhIndex *index, uint64_t *lo, uint64_t *hi);
bool smh_index_all_scaled(const SmhIndex *index);
int smh_downsample_block_dev(const uint64_t *hashes_dev, const uint32_t *abunds_dev, const uint64_t *offsets, uint32_t n,
                             uint64_t max_hash, uint64_t *out_hashes_dev, uint32_t *out_abunds_dev, uint64_t capacity,
                             uint64_t *out_offsets, void *stream);
void smh_downsample_geometry(uint32_t *tile_elems, uint32_t *threads);

/* Matching records: which k-mers of every record of a batch a resident index knows, and which node each record belongs
 * to -- without a sketch per record and without an N x M matrix.  The reference crate has no counterpart, so the rules are
 * fixed here -- DESIGN.md 3.13, restated in tests/match_restatement.py.  DNA only: a protein, dayhoff or hp index and
 * amino-acid input are not served.
 *   The index     must be uniform, DNA, every node a scaled sketch, with one max_hash; ksize, seed and max_hash are those of
 *                 node 0.  Anything else -- and an index without nodes -- is refused with SOURMASH_ERROR_CODE_MSG and a
 *                 message naming the node and the values, as smh_index_downsample refuses.  An index that
 *                 smh_index_downsample made is an index like any other.
 *   A window      of record r is a start position p with p + ksize <= end of r.  A window holding a byte outside ACGTacgt is
 *                 skipped (force = true semantics; never an error here).  A window never spans two records.
 *   Sampled       a window is sampled when the hash h of its canonical k-mer satisfies h <= max_hash (unsigned, inclusive).
 *   Hit           a sampled window is a hit when h is held by at least one node of the index.
 *   SmhMatchRow   per record: windows = sampled windows; distinct = distinct sampled hashes; hit_windows = sampled windows
 *                 that are hits; hit_distinct = distinct hit hashes; best = the node holding the most of the record's
 *                 distinct hit hashes, the lowest index on ties, 0xffffffff when hit_distinct == 0; best_common = that count
 *                 (by construction count_common(sketch(record), node best)).
 *   The hit list  optional: a CSR of every record's distinct hit hashes, ascending.  hit_offsets (caller's, n + 1 entries)
 *                 receives the offsets; *hit_hashes a malloc'ed array of *n_hits hashes (at least one element is allocated;
 *                 free it with free(), as smh_intersection's common_out).  Pass all three or none (NULL).
 * Every output is an integer: parity is equality.
 *
 * smh_index_match_sequences      records in host memory: seq + offsets[0 .. n] (record r = seq[offsets[r] .. offsets[r + 1])).
 * smh_index_match_sequences_dev  the batch in device memory (total_len bytes), offsets on the host; stream: the caller's.
 * smh_index_match_records        the records of an SmhRecords handle (they stay in HBM).
 *                                rows: room for n records.  The first call builds the index's hash directory (the sorted
 *                                distinct hashes of all nodes and the nodes holding each; fewer than 2^31 resident hashes)
 *                                and keeps it with the index; smh_index_free and smh_release_workspace give it back.
 * smh_match_geometry             the sizes at which the kernels' branches change: the owner pairs (hit hashes x the nodes
 *                                holding them) of one record up to which the tally counts in LDS -- a record with more goes
 *                                through per-node counters in global memory --, the threads the tally gives a record, and the
 *                                hashes of the directory the probe samples into LDS (a directory up to that size is searched
 *                                in LDS alone).
 * smh_match_set_pair_budget      bounds the work space that grows with the batch: a batch is cut into folds at record
 * smh_match_pair_budget          boundaries so that a fold's records plus its expected sampled windows stay within the budget
 *                                (one record always makes a fold: no record is split; a record that alone would leave 2^31
 *                                candidates is refused, MSG), and the dense regime of the tally serves as many records per
 *                                round as the budget holds (record, node) counters for (one at least).  Results never depend
 *                                on it.  0 restores the default, 2^26: a memory cap, not a measured optimum.  Process-wide.
 * Timers under smh_profile_get: "match_probe", "match_tally"; event counters: "match_directory_built", "match_fold",
 * "match_dense_round". */
typedef struct SmhMatchRow {
  uint32_t windows, distinct, hit_windows, hit_distinct, best, best_common;
} SmhMatchRow;
int smh_index_match_sequences(SmhIndex *index, const char *seq, const uint64_t *offsets, uint32_t n_records, SmhMatchRow *rows,
                              uint64_t *hit_offsets, uint64_t **hit_hashes, uint64_t *n_hits);
int smh_index_match_sequences_dev(SmhIndex *index, const void *seq_dev, uint64_t total_len, const uint64_t *offsets,
                                  uint32_t n_records, SmhMatchRow *rows, uint64_t *hit_offsets, uint64_t **hit_hashes,
                                  uint64_t *n_hits, void *stream);
int smh_index_match_records(SmhIndex *index, const SmhRecords *records, SmhMatchRow *rows, uint64_t *hit_offsets,
                            uint64_t **hit_hashes, uint64_t *n_hits);
void smh_match_geometry(uint32_t *lds_pairs, uint32_t *threads_per_record, uint32_t *probe_samples);
void smh_match_set_pair_budget(uint64_t pairs);
uint64_t smh_match_pair_budget(void);

/* Taxonomic LCA: what a sketch or a read is taxonomically, answered on the resident index (`lca classify`, `lca summarize`,
 * per-read screening).  The reference crate has no LCA code, so the rules are fixed here -- DESIGN.md 3.15, restated in
 * tests/lca_restatement.py.
 *   Taxonomy       parent[0 .. n_taxa), 1 <= n_taxa < 2^32 - 1.  Taxon 0 is the root and parent[0] == 0; parent[t] < t for
 *                  t > 0 (topological order).  node_taxon[0 .. n_nodes) gives each node's taxon; SMH_NO_TAXON marks a node
 *                  without a lineage, and such nodes are ignored everywhere below.
 *   lca(a, b)      the deepest common ancestor; SMH_NO_TAXON is its identity.
 *   A resident     hash has the taxon lca over the taxa of all nodes holding it, SMH_NO_TAXON when none of them has one.  A
 *   hash           query hash is ASSIGNED when the index holds it and its taxon is not SMH_NO_TAXON.
 *   Counts         of a sketch: the multiset of the taxa of its assigned hashes, reported as (taxon, count) pairs, taxon
 *                  ascending.  No roll-up to ancestors and no abundance weighting happen on the device.
 *   Classification of a set S of taxa (sourmash's find_lca on the tree built from the lineages): take the union of the root
 *                  paths of S and descend from the root while the current node has exactly one child in that union; the
 *                  result is the node where the descent stops.  status = 1 (found) when nothing lies below, 2 (disagree)
 *                  when it stopped at a branching; status = 0 and taxon SMH_NO_TAXON for the empty S.  This is not lca(S):
 *                  for S = {B, C} with B an ancestor of C the answer is C, found.
 *   Join           the classification is the fold of an associative, commutative join on summaries (x, f), f = disagree: a
 *                  taxon alone is (t, false).  With x the shallower operand: lca(x, y) != x gives (lca(x, y), true);
 *                  x == y gives (x, fx | fy); otherwise x is a strict ancestor of y and the result is (x, true) if fx, else
 *                  (y, fy).
 *   A record       is classified by S = the taxa of its distinct assigned hit hashes: every hit counts (`lca classify
 *                  --threshold 1`).  Windows, sampled windows, hits and record boundaries are those of "Matching records",
 *                  word for word.  Thresholds above 1 belong to the sketch route: the caller applies them to the counts.
 * Every output is an integer: parity is equality.  No result depends on chunking, budgets, launch geometry or the order of
 * atomics.
 *
 * smh_lca_check_taxonomy     the refusals of a taxonomy alone (SOURMASH_ERROR_CODE_MSG, the message names the offending
 *                            entry): n_taxa == 0 or 2^32 - 1; n_nodes != index_len; parent[0] != 0; parent[t] >= t; a node
 *                            taxon >= n_taxa that is not SMH_NO_TAXON.  Needs no device and no index.
 * smh_index_set_taxonomy     checks the arrays as above (index_len = smh_index_len) and copies them; host only.  Setting it
 *                            again replaces it and drops the per-hash table.
 * smh_index_has_taxonomy     an index smh_index_downsample makes from an index with a taxonomy carries the same taxonomy
 *                            (same nodes, same order).  An index without one is refused by the calls below (MSG).
 * smh_index_lca_many         the counts of every query of a batch.  count_offsets (the caller's, n_queries + 1 entries): the
 *                            pairs of query q are (*taxa)[count_offsets[q] .. count_offsets[q + 1]) (u32) with *counts (u64);
 *                            both are malloc'ed (at least one element) and freed with free().  query_offsets (nullable,
 *                            n_queries + 1): the running sum of the queries' sizes.  hash_taxon (nullable): one u32 per query
 *                            position in ascending hash order, the taxon of that hash or SMH_NO_TAXON.  Every query is
 *                            checked as smh_index_gather_many checks it; the error of the LOWEST failing query is reported
 *                            and nothing is written.  The index's nodes must be scaled sketches that agree in ksize,
 *                            molecule, seed and max_hash (else MSG).  A query that lives in HBM is staged device to device.
 * smh_index_lca_block_dev    the CSR / device form, as smh_index_gather_block_dev: hashes ascend strictly inside a query,
 *                            q_offsets on the host, hash_taxon counts from q_offsets[0]; stream: the caller's.
 * smh_index_lca_sequences    the three routes of "Matching records"; rows: one SmhLcaRow per record.  windows, distinct and
 * smh_index_lca_sequences_dev hit_distinct are SmhMatchRow's of the same record; assigned_distinct = the distinct assigned hit
 * smh_index_lca_records      hashes; taxon / status = the classification.  The index is refused as match refuses it.
 * smh_lca_geometry           the sizes at which the kernels' branches change: the owners of a hash up to which one lane
 *                            computes its taxon (a longer list gets a wave), the distinct sampled hashes of a record up to
 *                            which one lane classifies it (a longer record gets a wave), and the threads of that wave.
 * smh_lca_set_budget         the keys (query hashes) one chunk of a sketch batch may hold: chunks are cut at query boundaries
 * smh_lca_budget             and a query alone always makes a chunk.  0 restores the default of 2^26 -- a memory cap, not a
 *                            measured optimum.  Process-wide; results never depend on it.  The records route keeps using
 *                            smh_match_pair_budget for its folds.
 * The per-hash table (one taxon per distinct resident hash) is computed by the first device call after the taxonomy is set,
 * kept beside the hash directory and dropped with it (smh_release_workspace, smh_index_free) and by smh_index_set_taxonomy.
 * Timers under smh_profile_get: "lca_table", "lca_probe", "lca_records"; event counters: "lca_table_built", "lca_chunk",
 * and "match_directory_built" as before. */
#define SMH_NO_TAXON 0xffffffffu
typedef struct SmhLcaRow {
  uint32_t windows, distinct, hit_distinct, assigned_distinct, taxon, status;
} SmhLcaRow;
int smh_lca_check_taxonomy(const uint32_t *parent, uint32_t n_taxa, const uint32_t *node_taxon, uint32_t n_nodes,
                           uint32_t index_len);
int smh_index_set_taxonomy(SmhIndex *index, const uint32_t *parent, uint32_t n_taxa, const uint32_t *node_taxon,
                           uint32_t n_nodes);
bool smh_index_has_taxonomy(const SmhIndex *index);
int smh_index_lca_many(SmhIndex *index, const KmerMinHash *const *queries, uint32_t n_queries, uint64_t *count_offsets,
                       uint32_t **taxa, uint64_t **counts, uint64_t *query_offsets, uint32_t *hash_taxon);
int smh_index_lca_block_dev(SmhIndex *index, const uint64_t *q_hashes_dev, const uint64_t *q_offsets, uint32_t n_queries,
                            uint64_t *count_offsets, uint32_t **taxa, uint64_t **counts, uint32_t *hash_taxon, void *stream);
int smh_index_lca_sequences(SmhIndex *index, const char *seq, const uint64_t *offsets, uint32_t n_records, SmhLcaRow *rows);
int smh_index_lca_sequences_dev(SmhIndex *index, const void *seq_dev, uint64_t total_len, const uint64_t *offsets,
                                uint32_t n_records, SmhLcaRow *rows, void *stream);
int smh_index_lca_records(SmhIndex *index, const SmhRecords *records, SmhLcaRow *rows);
void smh_lca_geometry(uint32_t *owner_lane_max, uint32_t *record_lane_max, uint32_t *threads);
void smh_lca_set_budget(uint64_t keys);
uint64_t smh_lca_budget(void);

/* The kernels of the resident index (gather, gather_many, match, search_many, cluster, lca, collapse, index build) that walk
 * their items in a grid-stride loop are launched with min(ceil(items / items per workgroup), a limit of the launch's own)
 * workgroups -- on a large device the second trip through such a loop begins only at hundreds of thousands of items.
 * smh_set_grid_cap lowers every one of those grids to at most `workgroups`, so that tests reach the later trips, and the
 * state the kernels carry from trip to trip, at shapes of a few hundred items: 1 makes one workgroup take every trip.
 * 0 restores the default (no cap).  Process-wide, like the budgets; NO result depends on it -- it only slows large inputs
 * down, so set it around small ones.  Kernels that place their work by workgroup number alone keep their grids.  Every
 * launch whose grid the cap lowered adds one to the event counter "grid_capped" (smh_profile_get). */
void smh_set_grid_cap(uint32_t workgroups);
uint32_t smh_grid_cap(void);

/* deterministic synthetic DNA of SURVEY.md 8d written to device memory (benchmark input).  With a caller's stream the kernel
 * is left queued on it (the third exception of this header's opening contract: the benchmark queues it in front of
 * smh_add_sequences_dev on the same stream); with NULL the buffer is complete on return. */
int smh_synth_dna_dev(void *out_dev, uint64_t start, uint64_t len, uint64_t seed, uint64_t n_every,
                      void *stream);

/* The fold's sort on its own (diagnostic entry point for the parity tests): sorts `n` keys in host memory in place,
 * stably, carrying `payload` (n 32-bit values, or NULL) along -- on the device, through the same code as the sketch
 * fold and the compare pre-pass. */
int smh_sort_u64(uint64_t *keys, uint32_t *payload, uintptr_t n);

/* Which kernel serves an N x M compare block is chosen from the block's shape (a wavefront per
 * pair, a few-against-many stream, a per-component pair kernel, the tiled matrix kernel).  The
 * choice NEVER changes a result.  It can be pinned: the parity tests run every route over the same
 * inputs, and a caller that knows its collection is one big component can skip the pair route. */
enum SmhCompareRoute {
  SMH_ROUTE_AUTO = 0, SMH_ROUTE_WAVE = 1, SMH_ROUTE_FEW = 2, SMH_ROUTE_COMPONENTS = 3, SMH_ROUTE_TILED = 4
};
typedef struct SmhCompareTuning {
  uint32_t route;             /* SmhCompareRoute; default AUTO */
  uint32_t visit_all_tiles;   /* tiled route: 1 = launch every tile, not only those that can hold pairs sharing a hash */
  uint32_t use_symmetry;      /* default 1: all-vs-all with one num computes the upper triangle and mirrors it */
  uint64_t comp_pairs_limit;  /* AUTO: at most this many sharing pairs -> per-component pair kernel (default 96 Ki; the library
                                 lowers it to 16 Ki for a dictionary that carries range masks) */
  uint32_t split_frequent;    /* default 1: hashes held by more than a quarter of the sketches (at most 64 of them) do not
                                 connect sketches; pairs that share only such hashes are decided from per-sketch records
                                 instead of being walked */
  uint32_t dictionary;        /* how the pooled hashes of the collection dictionary are sorted: 0 = default (four radix passes over the
                                 32 most significant bits that vary, then the few keys that tie there are put in order), 1 = all
                                 eight byte passes (what the default falls back to; A/B and parity tests: same matrix either way) */
  uint32_t no_range_masks;    /* 1 = the tiled kernel walks every pair from the first range of rank space on; default 0: per-range
                                 bit masks of the shared hashes tell it where a pair's union reaches its cut, and it walks only
                                 from there (same matrix either way) */
} SmhCompareTuning;
void smh_compare_get_tuning(SmhCompareTuning *out);
int smh_compare_set_tuning(const SmhCompareTuning *tuning);   /* NULL restores the defaults; process-wide */

/* What the last block compare did.  Measurement aid and test evidence (which route ran; whether the
 * tiled kernel's global-memory merge branch was taken). */
typedef struct SmhCompareStats {
  uint32_t route;               /* SmhCompareRoute that ran */
  uint32_t rows_per_tile;       /* tiled route */
  uint64_t tiles_visited;       /* tiled: tiles launched; components: pairs walked */
  uint64_t tiles_total;         /* tiled: tiles in the block; components: pairs in the block */
  uint64_t pairs_per_tile;
  uint64_t lds_overflow_steps;  /* tiled: (tile, range) steps merged from global memory instead of the LDS stage */
  uint32_t frequent_hashes;     /* hashes set aside as frequent in this block (0 = none, or too many to set aside) */
  uint32_t pipelined;           /* tiled: 1 = the software-pipelined kernel walked the tiles (blocks that do not fill the chip for long) */
  uint32_t span_halvings;       /* pipelined kernel: stretches whose speculatively grown span did not fit LDS and was rebuilt, halved */
  uint32_t prefetched_after_halving; /* ... tiles in which prefetched boundary crossings were used after such a rebuild */
} SmhCompareStats;
void smh_compare_last_stats(SmhCompareStats *out);
/* 1 = the tiled kernel of the last block compare read the range masks ("Range masks"); 0 = it walked every range
 * from the first on, or another route served the block.  Whether a dictionary carries masks is decided when it is built: one
 * built under no_range_masks = 1 walks for its whole life, also under later default tunings.  (Kept out of SmhCompareStats,
 * which has no size field.) */
uint32_t smh_compare_last_range_masks(void);

/* The library keeps its device workspace (candidate buffers, the six-frame residue buffer, sort
 * scratch) between calls and only ever grows it; a long-running process can hand the memory back
 * after a large batch.  Sketches, resident indexes and their device copies are not touched. */
int smh_release_workspace(void);
/* Device blocks the library gives up (sketch buffers, mirrors, workspace) are parked in a pool inside the library, per
 * device and size class, instead of hipFree'd: another allocator in the process (PyTorch's) cannot see that memory.
 * The pool is capped (default 1 GiB; environment SOURMASH_AMD_POOL_MB=<MiB> at load time, 0 = no pooling); this call
 * changes the cap at run time (and trims down to it), smh_pool_bytes reports what is parked right now, and
 * smh_release_workspace() empties the pool together with the workspace. */
void smh_pool_set_limit(uint64_t bytes);
uint64_t smh_pool_bytes(void);
/* A test knob for what device work space holds before the library writes it.  Every byte of device memory the library
 * uses comes from that pool's allocator: new memory reads zero, a recycled block reads whatever it last held -- usually
 * the values the same operation left there, which are often right by accident.  With byte = 0 .. 255 every block the
 * allocator hands out, fresh or recycled, and every block it parks is first filled with that byte over its whole size
 * (hipMemset and a wait for the device: slow, for tests only); each fill adds one to the event counter "pool_filled"
 * (smh_profile_get).  -1 (any value outside 0 .. 255) turns it off, the default; then allocation takes exactly the path it
 * takes without this knob.  Process-wide; nothing reads an environment variable.  NO result depends on it: a result that
 * changes under a fill byte has read work space nobody wrote, or memory that was given back.  Blocks that are already in
 * use when the knob is set keep their content: smh_release_workspace() first, then the fill, then new objects, leaves no
 * library-owned block unfilled. */
void smh_set_pool_fill(int32_t byte);
int32_t smh_pool_fill(void);

/* Nodegraph (reference src/index/nodegraph.rs): a khmer-style bloom filter of n_tables bit tables, hash h sets bit
 * h % tablesize of each.  Single-hash calls and file I/O run on the host; count_many / get_many on the device.
 * Table sizes must be 1 .. 2^32 - 1.  count_many leaves the two counters exactly as count() called on the hashes in
 * array order would; out_new / out (nullable for count_many) receive one byte per hash.  load_* keep the header's
 * n_occupied and set unique_kmers to 0; a bad magic, version, table type or a short file is an error.  save_buffer
 * writes the reference's layout, including its quirk: a table whose size is a multiple of 8 is written one byte
 * shorter than the reader reads (khmer's sizes are primes).  smh_nodegraph_tablesizes returns n_tables and fills
 * `out` (nullable).  smh_nodegraph_bins is the device modulo on its own: out[i * n_tables + t] = hashes[i] %
 * tablesizes[t]. */
typedef struct SmhNodegraph SmhNodegraph;
SmhNodegraph *smh_nodegraph_new(const uint64_t *tablesizes, uint32_t n_tables, uint32_t ksize);
void smh_nodegraph_free(SmhNodegraph *ng);
SmhNodegraph *smh_nodegraph_load_buffer(const char *data, uint64_t len);
SmhNodegraph *smh_nodegraph_load_path(const char *path);
SourmashStr smh_nodegraph_save_buffer(const SmhNodegraph *ng);
bool smh_nodegraph_count(SmhNodegraph *ng, uint64_t hash);
int smh_nodegraph_count_many(SmhNodegraph *ng, const uint64_t *hashes, uint64_t n, uint8_t *out_new);
uint32_t smh_nodegraph_get(const SmhNodegraph *ng, uint64_t hash);
int smh_nodegraph_get_many(const SmhNodegraph *ng, const uint64_t *hashes, uint64_t n, uint8_t *out);
int smh_nodegraph_update(SmhNodegraph *ng, const SmhNodegraph *other);
double smh_nodegraph_similarity(const SmhNodegraph *ng, const SmhNodegraph *other);
double smh_nodegraph_containment(const SmhNodegraph *ng, const SmhNodegraph *other);
uint32_t smh_nodegraph_tablesizes(const SmhNodegraph *ng, uint64_t *out);
uint64_t smh_nodegraph_n_occupied_bins(const SmhNodegraph *ng);
uint64_t smh_nodegraph_unique_kmers(const SmhNodegraph *ng);
int smh_nodegraph_bins(const uint64_t *tablesizes, uint32_t n_tables, const uint64_t *hashes, uint64_t n, uint32_t *out);

/* Sequence Bloom Tree (reference src/index/sbt.rs, MHBT = SBT<Node<Nodegraph>, Leaf<Signature>>), resident in HBM:
 * every internal nodegraph (they share one set of table sizes) plus the leaves' first sketches.
 *   load_path  a v5 JSON; storage = the JSON's directory joined with storage.args.path (nodes: OXLI files, leaves:
 *              signature files whose first sketch of the first signature is the leaf's data).
 *   build      leaves at the given positions of a d-ary tree; every ancestor position gets an internal node holding
 *              the bloom filter of the leaves below it, min_n_below = the smallest leaf size below it, n_occupied =
 *              popcount of table 0 (what a khmer file carries), unique_kmers = 0.
 *   save       json_path (NAME.sbt.json) + the directory .sbt.NAME beside it: internal.POS nodegraphs and leaf signatures.
 *   find       SBT::find with search_minhashes (containment false) or search_minhashes_containment: the positions of the
 *              leaves that pass, in the reference's walk order; out_positions holds n_leaves entries.  A query
 *              incompatible with a leaf the walk reaches is error 101-104; a node without min_n_below reached by a
 *              non-empty query in similarity mode is an error.
 *   find_many  the same for n queries at once: query i's list is positions[offsets[i] .. offsets[i + 1]); out_offsets
 *              holds n + 1 entries, *out_positions points into the tree's own storage (valid until the next find on it).
 * leaf_positions: ascending positions of the leaves (n_leaves entries); leaf_sketch(i) is a copy of leaf i's sketch in
 * that order (free it with kmerminhash_free). */
typedef struct SmhSbt SmhSbt;
SmhSbt *smh_sbt_load_path(const char *json_path);
SmhSbt *smh_sbt_build(uint32_t d, const uint64_t *positions, KmerMinHash *const *leaves, uint32_t n_leaves,
                      const uint64_t *tablesizes, uint32_t n_tables, uint32_t ksize);
int smh_sbt_save(const SmhSbt *sbt, const char *json_path);
void smh_sbt_free(SmhSbt *sbt);
uint32_t smh_sbt_n_nodes(const SmhSbt *sbt);
uint32_t smh_sbt_n_leaves(const SmhSbt *sbt);
int smh_sbt_leaf_positions(const SmhSbt *sbt, uint64_t *out);
KmerMinHash *smh_sbt_leaf_sketch(const SmhSbt *sbt, uint32_t i);
int smh_sbt_find(SmhSbt *sbt, const KmerMinHash *query, double threshold, bool containment, uint64_t *out_positions,
                 uint32_t *out_count);
int smh_sbt_find_many(SmhSbt *sbt, KmerMinHash *const *queries, uint32_t n, double threshold, bool containment,
                      uint64_t *out_offsets, const uint64_t **out_positions);

/* HIP-event timing of the library's kernels, on the stream they run on.
 * name: "dna_rolling", "dna_generic", "protein_fused", "translate", "hash_windows", "compare_wave", "compare_few",
 * "compare_pair", "compare_fill", "compare_comp", "compare_tiled" (the plain and the pipelined tiled kernels of one call together),
 * "sbt_bins", "sbt_nodes", "sbt_leaves", "sbt_build", "parse_scan" (tile summaries and their scan), "parse_compact",
 * "gather_hits" (the membership pass), "gather_invert" (degree scan + inverted lists), "gather_rounds" (one entry per batch
 * of smh_gather_rounds_per_sync() rounds), "angular_block" (the angular similarity's block kernel), "match_probe" (the runs of a
 * fold against the hash directory), "match_tally" (the per-record tally: its LDS launch, and one entry per dense round),
 * "gather_many_probe" (a chunk's probe, counts and sizing), "gather_many_fill" (the scan and the hit lists),
 * "gather_many_rounds" (one entry per batch of smh_gather_rounds_per_sync() rounds of a chunk), "search_many_probe" (a
 * chunk's probe), "search_many_select" (the rule on every counter, the counts per tile and their scan), "search_many_emit" (the
 * rows of a chunk), "cluster_probe" (a chunk's upper-triangle probe), "cluster_link" (the rule on every counter above the
 * diagonal, a union per survivor), "cluster_finish" (labels, representatives and the numbering), "cluster_round" (one entry
 * per greedy round), "cluster_assign" (the members' choice), "collapse_count" / "collapse_emit" (the two folds of the
 * directory's owner lists through the groups, three launches each), "collapse_partition" (the survivors sorted by group and
 * the groups' bounds among them), "collapse_finish" (the child's hashes and abundances from the partitioned survivors),
 * "filter_flag" (a filter's verdict per resident hash and the survivors per tile), "filter_emit" (its survivors written in
 * order), "nearest_clamp" (the candidates kept per tile and the rows per query, and their scan), "nearest_tile" (a tile's
 * survivors sorted in LDS, its best k kept), "nearest_merge" (a query's candidates folded into its best k, and its rows).
 * Event counters under the same call: "gather_many_chunk",
 * "search_many_chunk", "nearest_chunk", "cluster_chunk" (chunks run), "cluster_round" (greedy rounds launched; with the timers enabled their
 * entries are that count), "match_directory_built", "index_collapsed", "index_filtered", "index_selected", "grid_capped"
 * (launches whose grid smh_set_grid_cap lowered), "pool_free_waited" (device blocks given back behind a wait for the whole
 * device). */
void smh_profile_enable(int on);
void smh_profile_reset(void);
int smh_profile_get(const char *name, double *total_ms, uint64_t *launches);

/* Signature JSON on the device.  A database arrives as `.sig` JSON, and nearly all of its bytes are decimal
 * digits inside `mins` and `abundances`.  An SmhSignatures handle is made from such text in host or device memory: the DEVICE
 * turns every number of every numeric array into u64 and keeps them in HBM in document order; the HOST receives the span table
 * of those arrays and the text without them -- a skeleton of a few hundred bytes per signature -- which it parses with the
 * JSON parser of the host loader, so keys, nulls, defaults, Q9, unknown fields and escapes mean what they mean there.  An index
 * of chosen sketches is then built with device-to-device copies: nothing proportional to the hashes crosses to the host in
 * either direction.  The rules (tests/sigscan_restatement.py states them as plain Python and is normative):
 *   String state   a byte is inside a string if an odd number of unescaped '"' precede it; a '"' is escaped if it is directly
 *              preceded by an odd-length run of '\'.
 *   Span       every '[' outside a string opens a span: the maximal run of bytes from 0-9 ',' ' ' '\n' '\t' '\r' directly
 *              behind it (it may be empty).  The k-th such '[' of the text owns span k.
 *   Tokens     a token is a maximal digit run inside a span; its value is values[first_token[k] + i].  A token that breaks
 *              a rule below has the value 0.
 *   Status     of a span; the lowest rule broken decides and the offset of the offending byte is kept:
 *              SMH_SIGSPAN_BAD_SYNTAX   a comma whose previous non-blank byte in the span is not a digit (the comma);  a token
 *                                       whose previous non-blank byte in the span is a digit (its first digit);  a token of more
 *                                       than one digit that starts with 0 (that 0);
 *              SMH_SIGSPAN_OVERFLOW     a token above 2^64 - 1 (its first digit), which any token of more than 20 digits is: at
 *                                       most 21 digits of a token are read, however long it is;
 *              SMH_SIGSPAN_OPEN         the last non-blank byte is a comma;
 *              SMH_SIGSPAN_CLOSED       otherwise.
 *   Skeleton   the text with every span's bytes removed: behind every '[' stands its hole.
 *   Host       the k-th '[' of the skeleton gets span k's tokens as its leading elements.  OPEN must be followed by a value;
 *              CLOSED with tokens by ']'; CLOSED without tokens by either.  BAD_SYNTAX fails the document wherever the array
 *              stands; OVERFLOW fails only an array read as u64 (`mins`, `abundances`: elsewhere such a number reads as a
 *              float).  An array read as u64 must consist of its span alone.  A span that reaches its document's end fails
 *              that document.
 *   Deviation  a span that ends in a digit and is followed in the skeleton by '.', 'e' or 'E' is a float split in two.  The
 *              call refuses the document with code 3, names the document and the byte offset and points to load_signatures.
 *              No sourmash writer produces this.
 * Documents: text[doc_offsets[d], doc_offsets[d + 1]) is document d, a JSON array of signatures as signatures_load_buffer takes
 * one; doc_offsets == NULL: the whole text is one document (n_docs is not read).  The documents tile the text: doc_offsets
 * ascend, doc_offsets[0] == 0 and doc_offsets[n_docs] == len, else code 3 (the scan enters byte 0 outside a string, so bytes
 * that belong to no document would decide how the documents behind them are read).  A document is accepted exactly when
 * signatures_load_buffer accepts it, apart from the deviation.  Where both refuse the code is 100004 (serde); the message begins
 * "document D, byte B: " (B counts in the document's own text); the lowest failing document decides and no handle is returned.
 * An accepted document's metadata equals the host loader's field for field (`num` follows Q9).
 * Entries: one per sketch, in document order, then signature order, then sketch order -- the order signatures_load_buffer
 * flattens them in.  smh_signatures_entry fills an SmhSigEntry; its strings are NUL-terminated, owned by the handle and valid
 * while it lives; `md5sum` is the string as written (it is not verified).  smh_signatures_span gives one row of the span
 * table (any pointer may be NULL); smh_signatures_values_dev the values in HBM, smh_signatures_tokens of them.
 * smh_signatures_parse uploads host text once and parses it; *_parse_dev takes text already in HBM at any alignment, follows
 * the stream contract at the top of this file and reads no byte outside [text, text + len).  Both return complete.
 *   smh_signatures_index            node j = the `mins` of entry ids[j]: any order, repeats allowed, ids == NULL: every entry
 *              (n_ids is not read).  The per-node parameters, whether the index has abundances (every node has them, as many as
 *              hashes), their narrowing to 32 bits and the places of abundances of 2^32 or more are decided as smh_index_new
 *              decides them, so the result answers every call as smh_index_new(signatures_load_buffer(...)) does.  One refusal
 *              of its own, code 3: the hashes of every chosen sketch must be strictly ascending (the compare kernels assume
 *              it); the message names the lowest node and position, and nothing is built.
 *   smh_signatures_filter           the entries signatures_load_buffer's filter keeps (ksize 0: any; moltype NULL: any, else
 *              "dna", "protein", "dayhoff" or "hp" in any case; any other string keeps none), ascending: returns how many and,
 *              when ids_out is not NULL, writes them (room for smh_signatures_len entries always suffices).  Needs no device.
 *   smh_signatures_index_filtered   smh_signatures_index of exactly those entries.
 * Out of scope: single-stream gzip on the device outside a zip collection (BGZF goes through smh_gzip_inflate_dev in front of
 * *_parse_dev, a zip collection through smh_archive_inflate_dev: "Zip collections"), md5 verification, sorting unsorted `mins`.  (Writing signatures: the next section.)
 * smh_sigscan_geometry: bytes per workgroup tile (cut on 16-byte boundaries of the address) and threads per workgroup (tests,
 * tools).  Timers: "sigscan_summary", "sigscan_scan", "sigscan_compact", "sigscan_gather" (the checks of a gathered index; its
 * copy is timed as "downsample_copy"); event counters: "signatures_parsed", "index_from_signatures". */
typedef struct SmhSignatures SmhSignatures;
enum { SMH_SIGSPAN_CLOSED = 0, SMH_SIGSPAN_OPEN = 1, SMH_SIGSPAN_OVERFLOW = 2, SMH_SIGSPAN_BAD_SYNTAX = 3 };
typedef struct SmhSigEntry {
  uint32_t document, signature, sketch;   /* where the sketch stands in the text */
  uint32_t num, ksize;
  uint64_t seed, max_hash;
  int32_t molecule;                       /* SMH_MOLECULE_* */
  uint8_t name_is_null, filename_is_null; /* the JSON null (or the key is missing): the string is then "" */
  uint8_t has_abundances;                 /* `abundances` is present and not null */
  uint8_t pad;
  const char *name, *filename, *license, *sig_class, *md5sum;
  uint64_t n_mins, n_abundances;          /* tokens of the two arrays */
  uint64_t mins_span, abundances_span;    /* their rows in the span table (abundances_span: only with has_abundances) */
} SmhSigEntry;
SmhSignatures *smh_signatures_parse(const char *text, uint64_t len, const uint64_t *doc_offsets, uint32_t n_docs);
SmhSignatures *smh_signatures_parse_dev(const void *text_dev, uint64_t len, const uint64_t *doc_offsets, uint32_t n_docs, void *stream);
void smh_signatures_free(SmhSignatures *sigs);
uint32_t smh_signatures_len(const SmhSignatures *sigs);      /* entries */
uint64_t smh_signatures_spans(const SmhSignatures *sigs);
uint64_t smh_signatures_tokens(const SmhSignatures *sigs);
int smh_signatures_entry(const SmhSignatures *sigs, uint32_t i, SmhSigEntry *out);
int smh_signatures_span(const SmhSignatures *sigs, uint64_t k, uint64_t *start, uint64_t *end, uint64_t *first_token, uint64_t *n_tokens,
                        uint32_t *status, uint64_t *bad_offset /* all ones: none */);
const uint64_t *smh_signatures_values_dev(const SmhSignatures *sigs);   /* device */
SmhIndex *smh_signatures_index(const SmhSignatures *sigs, const uint32_t *ids, uint32_t n_ids);
uint32_t smh_signatures_filter(const SmhSignatures *sigs, uint64_t ksize, const char *moltype, uint32_t *ids_out);
SmhIndex *smh_signatures_index_filtered(const SmhSignatures *sigs, uint64_t ksize, const char *moltype);
void smh_sigscan_geometry(uint32_t *tile_bytes, uint32_t *threads);

/* Signature JSON written on the device: the way out of a resident index.  An SmhSigText handle owns, in HBM,
 * the byte string signatures_save_buffer gives for the index's own sketches (what smh_index_read returns, with the per-node
 * parameters the index holds), each wrapped in a default Signature with the given name and filename; only 16 bytes per node
 * cross to the host, and the skeleton of a few hundred bytes per node goes the other way.  The rules
 * (tests/sigtext_restatement.py states them as plain Python and is normative):
 *   Text       the documents one after another, no separator; a document is [SIG,SIG,...] of its nodes, an empty one is [];
 *              compact serde_json: no blanks, no newline.
 *   SIG        {"class":"sourmash_signature","email":"","hash_function":"0.murmur64","filename":F,"name":N,"license":"CC0",
 *              "signatures":[{"num":..,"ksize":..,"seed":..,"max_hash":..,"mins":[h,h,...],"md5sum":"<32 lower-case hex>"
 *              [,"abundances":[a,a,...]],"molecule":"DNA|protein|dayhoff|hp"}],"version":0.4}
 *   F, N       null or the string, escaped as the host writer escapes it (one function, sigjson.hpp's json_escape).
 *   abundances present on every node exactly when smh_index_has_abundances; the index's u32 values.
 *   md5sum     the MD5 of the decimal ksize followed by the decimal hashes, no separator (an empty node: of the ksize alone).
 * names / filenames: NULL = every one null; else n pointers, a NULL element = JSON null.  doc_starts: NULL = one document of all
 * nodes (n_docs is not read); else n_docs + 1 ascending node numbers, [0] == 0, [n_docs] == n.  Refusals, code 3 with a message
 * that begins "sigtext:", before anything is allocated: a bad doc_starts (the entry is named); an index that holds an abundance
 * of 2^32 or more (the node is named: the index no longer has its value).  Without a device: code 2.  Both calls return
 * complete, on the library's own stream.
 * smh_sigtext_doc_offsets writes documents + 1 offsets from 0 (what smh_signatures_parse_dev takes); smh_sigtext_dev is the text
 * in HBM, owned by the handle and valid while it lives; smh_sigtext_read copies text[offset, offset + len) to the host (a range
 * outside the text: code 3).  smh_index_md5 writes the 16 n digest bytes alone and builds no text.
 * Out of scope: compression of the output, writing zip containers, several sketches in one signature, `email`, `license` or `version`
 * other than the defaults.
 * smh_sigtext_geometry: values per workgroup tile of the measure and emit passes, threads per workgroup, values a wave formats
 * per step of the md5 pass (tests, tools).  Timers: "sigtext_measure", "sigtext_scan", "sigtext_emit", "sigtext_md5"; event
 * counter: "index_sigtext". */
typedef struct SmhSigText SmhSigText;
SmhSigText *smh_index_sigtext(SmhIndex *index, const char *const *names, const char *const *filenames, const uint32_t *doc_starts,
                              uint32_t n_docs);
uint64_t smh_sigtext_len(const SmhSigText *t);
uint32_t smh_sigtext_documents(const SmhSigText *t);
int smh_sigtext_doc_offsets(const SmhSigText *t, uint64_t *out);   /* documents + 1, from 0 */
const void *smh_sigtext_dev(const SmhSigText *t);                  /* device */
int smh_sigtext_read(const SmhSigText *t, uint64_t offset, uint64_t len, char *out);
void smh_sigtext_free(SmhSigText *t);
int smh_index_md5(SmhIndex *index, uint8_t *out);                  /* 16 n bytes */
void smh_sigtext_geometry(uint32_t *values_per_tile, uint32_t *threads, uint32_t *md5_values_per_step);

/* Zip collections: the container sourmash writes its databases in -- members signatures/<md5>.sig.gz, stored
 * in the zip because they are gzip already, and a SOURMASH-MANIFEST.csv -- read into HBM with the compressed bytes uploaded
 * once and every chosen member inflated on the device, each into its own slice of one text that smh_signatures_parse_dev
 * takes.  tests/archive_restatement.py states the scan and the CRC fold as plain Python and is normative.
 *   smh_archive_scan   reads data[0, len) on the host; no device is touched.  The end-of-central-directory record is looked
 *              for in the last 22 + 65535 bytes: a place counts when the signature PK\5\6 stands there AND its comment length
 *              leads exactly to the end of the data; the LOWEST such place is the record (a record spelled inside the comment
 *              stands behind the true one).  A zip64 locator directly in front of it leads to the zip64 end record, whose
 *              counts, size and offset then hold.  Every central-directory entry is read, with the zip64 extra field (id 1:
 *              size, compressed size, header offset, disk; each present only when its fixed field is all ones) for sizes and
 *              offsets; then the entry's local header, whose OWN name and extra lengths give the data offset (they may differ
 *              from the central directory's).  Sizes and the CRC-32 come from the central directory, so data descriptors
 *              (flag bit 3) are fine.  Offsets are taken as written: an archive with prepended data is out of scope.
 *              kind is decided from content, not from the name: a name ending '/' with size 0 is SMH_ARCHIVE_DIRECTORY;
 *              else method 8 is DEFLATE; method 0 whose data begins 1f 8b 08 is GZIP, other method 0 is STORED; any other
 *              method is OTHER.  A GZIP entry is treated as ONE gzip member: its RFC 1952 header is read as smh_gzip_scan
 *              reads one, without the BC requirement; the payload is everything up to the last 8 bytes, and CRC-32 and ISIZE
 *              come from that trailer.  (A multi-member .gz is not detected here: the decoder reports it as
 *              SMH_INFLATE_LEFTOVER, or as an output above or below ISIZE.)
 *              device_ok is 0, with a reason string, and the entry is still listed, for: an encrypted entry (flag bit 0); a
 *              method other than 0 or 8; a compressed or inflated size of 2^32 or more; a method-0 entry whose two sizes
 *              differ; a GZIP entry shorter than its header plus trailer.
 *              The whole archive is refused, code 3, with a message "archive: ... (entry I at byte B)" -- "(at byte B)" where
 *              no entry is meant -- for: no end record; a multi-disk archive (any disk number other than 0, or a count on
 *              this disk that is not the total); a zip64 end record outside the data or without its signature; a central
 *              directory outside the data in front of the end record; a truncated central directory (an entry that does not
 *              fit into the directory's announced size); a directory entry or a local header without its signature; a zip64
 *              extra field missing or cut short; a local header or entry data outside data[0, len).
 *   smh_archive_entry   fills an SmhArchiveEntry; its strings are NUL-terminated, owned by the handle and valid while it
 *              lives.  payload_off / payload_len: what a device inflate reads (the DEFLATE stream of a DEFLATE or GZIP entry,
 *              the bytes of a STORED one); text_size / text_crc: the size and CRC-32 of what it writes (GZIP: the trailer's
 *              ISIZE and CRC-32; else the central directory's).  Only meaningful with device_ok.
 *   smh_archive_inflate_dev   data_dev: the len scanned bytes in HBM at any alignment.  ids: n_ids entries, any order,
 *              repeats allowed; entry ids[i] becomes out[out_offs[i], out_offs[i] + text_size): the caller lays out the text.
 *              Refused before anything is launched, code 3: len other than the scanned length; an id past the entries or
 *              whose device_ok is 0; a slice that leaves out_cap; two non-empty slices that overlap.  It follows the stream
 *              contract at the top of this file and returns complete.  Members are inflated one wave each, handed out
 *              longest payload first from a ticket (members differ by orders of magnitude; a wave decodes a few MB/s); STORED
 *              members are copied.  verify: the CRC-32 of every text is taken in chunks of smh_archive_geometry's size spread
 *              over the device, folded per member and compared -- with the gzip trailer's for GZIP (the zip's CRC over a
 *              stored .gz's compressed bytes is not checked: the trailer covers the content), with the central directory's
 *              for DEFLATE and STORED.  verify = 0 skips it; stored members are still copied and sizes are always checked.
 *              status_out (host, one byte per id, or NULL) receives the SMH_INFLATE_* status of every position, also when
 *              the call fails.  A failing call returns code 3 with "archive: <reason> (entry I 'name')" for the LOWEST bad
 *              position of ids.  On ANY input no byte outside data[0, len) is read and none outside the given slices is
 *              written.  Offsets into the text are 64-bit everywhere.
 *   smh_archive_inflate   the same from host bytes, with one upload of the compressed file; on the library's own stream.
 * smh_archive_geometry: bytes per CRC chunk and threads per workgroup (tests, tools).  smh_archive_set_sorted(0) is a
 * measurement knob like smh_set_grid_cap: members are handed out in id order instead of longest first (default 1;
 * smh_archive_sorted reads it back).  It is one word of the process, read without a lock by every call: not thread-safe, not
 * for production use -- the result is the same either way, only the time differs.  Timers: "archive_inflate",
 * "archive_chunks", "archive_crc".
 * Out of scope: writing zips, SBT zips, FASTA / FASTQ inside zips, bzip2 / lzma / zstd methods, archives with prepended data. */
typedef struct SmhArchive SmhArchive;
enum { SMH_ARCHIVE_STORED = 0, SMH_ARCHIVE_DEFLATE = 1, SMH_ARCHIVE_GZIP = 2, SMH_ARCHIVE_DIRECTORY = 3, SMH_ARCHIVE_OTHER = 4 };
typedef struct SmhArchiveEntry {
  const char *name, *reason;              /* reason: why device_ok is 0, else "" */
  uint32_t method, flags, crc32, kind;    /* as the central directory has them; kind: SMH_ARCHIVE_* */
  uint32_t device_ok, text_size, text_crc, pad;
  uint64_t comp_size, size;               /* central directory, or its zip64 extra field */
  uint64_t header_off, data_off;          /* the local header; the entry's bytes are data[data_off, data_off + comp_size) */
  uint64_t payload_off, payload_len;
} SmhArchiveEntry;
SmhArchive *smh_archive_scan(const void *data, uint64_t len);
void smh_archive_free(SmhArchive *a);
uint64_t smh_archive_entries(const SmhArchive *a);
int smh_archive_entry(const SmhArchive *a, uint64_t i, SmhArchiveEntry *out);
int smh_archive_inflate_dev(const SmhArchive *a, const void *data_dev, uint64_t len, const uint32_t *ids, const uint64_t *out_offs,
                            uint64_t n_ids, void *out_dev, uint64_t out_cap, int verify, uint8_t *status_out /* host, or NULL */,
                            void *stream);
int smh_archive_inflate(const SmhArchive *a, const void *data, uint64_t len, const uint32_t *ids, const uint64_t *out_offs, uint64_t n_ids,
                        void *out_dev, uint64_t out_cap, int verify, uint8_t *status_out);
void smh_archive_geometry(uint32_t *chunk_bytes, uint32_t *threads);
void smh_archive_set_sorted(int sorted);
int smh_archive_sorted(void);

#ifdef __cplusplus
}
#endif
#endif
