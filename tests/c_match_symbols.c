/* Link check of the entry points that match records against a resident index (include/sourmash_amd.h, "Matching
 * records"): each is called with the header's prototype.  Needs no GPU: with one the three routes answer and agree, without
 * one every device call returns 2; the geometry and the budget need no device either way. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(void) {
  uint32_t lds_pairs = 0, threads = 0, samples = 0;
  smh_match_geometry(&lds_pairs, &threads, &samples);
  CHECK(lds_pairs > 0 && threads > 0 && threads % 64 == 0 && samples > 0);
  const uint64_t def = smh_match_pair_budget();
  CHECK(def > 0);
  smh_match_set_pair_budget(12345);
  CHECK(smh_match_pair_budget() == 12345);
  smh_match_set_pair_budget(0);
  CHECK(smh_match_pair_budget() == def);

  /* pyoracle.synth_dna(0, 30, 11) and the hash of its window 2 at k = 21 (tests/test_match_rules.py) */
  const char *rec = "CTCGAATAAAAGTAGACTTCACGCCCTTAAACGT";   /* + a second record of four bases */
  const uint64_t off[3] = {0, 30, 34}, planted = 2411703374284256564ull;
  const int have = smh_device_available();
  KmerMinHash *node = kmerminhash_new(0, 21, false, 42, UINT64_MAX, false);
  CHECK(node);
  kmerminhash_add_hash(node, planted);
  KmerMinHash *nodes[1] = {node};
  SmhIndex *index = smh_index_new(nodes, 1);
  CHECK((index != NULL) == (have != 0));
  sourmash_err_clear();
  SmhMatchRow rows[2];
  uint64_t hit_off[3] = {9, 9, 9}, *hits = NULL, n_hits = 9;
  memset(rows, 0xee, sizeof rows);
  const int rc = smh_index_match_sequences(index, rec, off, 2, rows, hit_off, &hits, &n_hits);
  CHECK(rc == (have ? 0 : 2));
  if (have) {
    CHECK(rows[0].windows == 10 && rows[0].distinct == 10 && rows[0].hit_windows == 1 && rows[0].hit_distinct == 1);
    CHECK(rows[0].best == 0 && rows[0].best_common == 1);
    CHECK(rows[1].windows == 0 && rows[1].hit_distinct == 0 && rows[1].best == 0xffffffffu && rows[1].best_common == 0);
    CHECK(n_hits == 1 && hits && hits[0] == planted && hit_off[0] == 0 && hit_off[1] == 1 && hit_off[2] == 1);
    free(hits);
    SmhRecords *parsed = smh_records_parse(">a\nCTCGAATAAAAGTAGACTTCACGCCCTTAA\n>b\nACGT\n", 42, 0);
    CHECK(parsed && smh_records_len(parsed) == 2);
    SmhMatchRow again[2], third[2];
    CHECK(smh_index_match_records(index, parsed, again, NULL, NULL, NULL) == 0);
    CHECK(memcmp(again, rows, sizeof rows) == 0);
    CHECK(smh_index_match_sequences_dev(index, smh_records_seq_dev(parsed), smh_records_total(parsed), smh_records_offsets(parsed), 2,
                                        third, NULL, NULL, NULL, NULL) == 0);
    CHECK(memcmp(third, rows, sizeof rows) == 0);
    smh_records_free(parsed);
  } else {
    CHECK(smh_index_match_records(index, NULL, rows, NULL, NULL, NULL) == 2);
    CHECK(smh_index_match_sequences_dev(index, NULL, 0, off, 2, rows, NULL, NULL, NULL, NULL) == 2);
  }
  sourmash_err_clear();
  smh_index_free(index);
  kmerminhash_free(node);
  printf("match abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
