/* Link check of the taxonomic LCA entry points (include/sourmash_amd.h, "Taxonomic LCA"): each is called with the header's
 * prototype.  Needs no GPU: with one a three-node index answers through plain C, without one every device call returns 2;
 * the taxonomy's checks, the geometry and the budget need no device either way. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(void) {
  uint32_t owner_lane_max = 0, record_lane_max = 0, threads = 0;
  smh_lca_geometry(&owner_lane_max, &record_lane_max, &threads);
  CHECK(owner_lane_max > 0 && record_lane_max > 0 && threads == 64);
  const uint64_t def = smh_lca_budget();
  CHECK(def > 0);
  smh_lca_set_budget(12345);
  CHECK(smh_lca_budget() == 12345);
  smh_lca_set_budget(0);
  CHECK(smh_lca_budget() == def);

  /*  0 - 1 - 2
   *        \ 3      nodes: taxon 2, taxon 3, no lineage */
  const uint32_t parent[4] = {0, 0, 1, 1}, node_taxon[3] = {2, 3, SMH_NO_TAXON}, bad_parent[3] = {0, 2, 1};
  CHECK(smh_lca_check_taxonomy(parent, 4, node_taxon, 3, 3) == 0);
  CHECK(smh_lca_check_taxonomy(bad_parent, 3, node_taxon, 3, 3) == 3);
  CHECK(smh_lca_check_taxonomy(parent, 4, node_taxon, 3, 2) == 3);
  sourmash_err_clear();
  CHECK(!smh_index_has_taxonomy(NULL));

  /* pyoracle.synth_dna(0, 30, 11) and the hash of its window 2 at k = 21 (tests/test_match_rules.py) */
  const char *rec = "CTCGAATAAAAGTAGACTTCACGCCCTTAAACGT";   /* + a second record of four bases */
  const uint64_t off[3] = {0, 30, 34}, planted = 2411703374284256564ull;
  const int have = smh_device_available();
  KmerMinHash *nodes[3], *query = kmerminhash_new(0, 21, false, 42, UINT64_MAX, false);
  for (int i = 0; i < 3; i++) CHECK((nodes[i] = kmerminhash_new(0, 21, false, 42, UINT64_MAX, false)) != NULL);
  /* planted: nodes 0 and 1 (taxa 2 and 3: lca 1); 5: node 0 (taxon 2); 7: node 2 alone (unassigned); 9: nobody */
  kmerminhash_add_hash(nodes[0], planted); kmerminhash_add_hash(nodes[1], planted);
  kmerminhash_add_hash(nodes[0], 5); kmerminhash_add_hash(nodes[2], 7);
  const uint64_t qh[4] = {5, 7, 9, planted};
  for (int i = 0; i < 4; i++) kmerminhash_add_hash(query, qh[i]);
  SmhIndex *index = smh_index_new(nodes, 3);
  CHECK((index != NULL) == (have != 0));
  sourmash_err_clear();

  const KmerMinHash *queries[2] = {query, query};
  uint64_t coff[3] = {9, 9, 9}, qoff[3] = {9, 9, 9}, *counts = NULL;
  uint32_t *taxa = NULL, per[8];
  SmhLcaRow rows[2];
  memset(rows, 0xee, sizeof rows);
  if (have) {
    CHECK(smh_index_lca_many(index, queries, 2, coff, &taxa, &counts, qoff, per) == 3);   /* no taxonomy yet */
    CHECK(coff[0] == 9 && taxa == NULL);
    CHECK(smh_index_lca_sequences(index, rec, off, 2, rows) == 3);
    CHECK(smh_index_set_taxonomy(index, parent, 4, node_taxon, 2) == 3);
    CHECK(!smh_index_has_taxonomy(index));
    sourmash_err_clear();
    CHECK(smh_index_set_taxonomy(index, parent, 4, node_taxon, 3) == 0);
    CHECK(smh_index_has_taxonomy(index));
    CHECK(smh_index_lca_many(index, queries, 2, coff, &taxa, &counts, qoff, per) == 0);
    CHECK(coff[0] == 0 && coff[1] == 2 && coff[2] == 4 && qoff[1] == 4 && qoff[2] == 8);
    CHECK(taxa[0] == 1 && counts[0] == 1 && taxa[1] == 2 && counts[1] == 1 && taxa[2] == 1 && taxa[3] == 2);
    CHECK(per[0] == 2 && per[1] == SMH_NO_TAXON && per[2] == SMH_NO_TAXON && per[3] == 1 && per[4] == 2 && per[7] == 1);
    free(taxa); free(counts);
    CHECK(smh_index_lca_sequences(index, rec, off, 2, rows) == 0);
    CHECK(rows[0].windows == 10 && rows[0].distinct == 10 && rows[0].hit_distinct == 1 && rows[0].assigned_distinct == 1);
    CHECK(rows[0].taxon == 1 && rows[0].status == 1);
    CHECK(rows[1].windows == 0 && rows[1].hit_distinct == 0 && rows[1].taxon == SMH_NO_TAXON && rows[1].status == 0);
    SmhRecords *parsed = smh_records_parse(">a\nCTCGAATAAAAGTAGACTTCACGCCCTTAA\n>b\nACGT\n", 42, 0);
    CHECK(parsed && smh_records_len(parsed) == 2);
    SmhLcaRow again[2], third[2];
    CHECK(smh_index_lca_records(index, parsed, again) == 0);
    CHECK(memcmp(again, rows, sizeof rows) == 0);
    CHECK(smh_index_lca_sequences_dev(index, smh_records_seq_dev(parsed), smh_records_total(parsed), smh_records_offsets(parsed), 2,
                                      third, NULL) == 0);
    CHECK(memcmp(third, rows, sizeof rows) == 0);
    /* the CSR form on hashes that already live in device memory: the records' bytes serve as two 8-byte "hashes" of one
     * query nobody holds -- zero pairs, no error */
    const uint64_t boff[2] = {0, 1};
    CHECK(smh_index_lca_block_dev(index, (const uint64_t *)smh_records_seq_dev(parsed), boff, 1, coff, &taxa, &counts, per, NULL) == 0);
    CHECK(coff[0] == 0 && coff[1] == 0 && per[0] == SMH_NO_TAXON);
    free(taxa); free(counts);
    smh_records_free(parsed);
    SmhIndex *child = smh_index_downsample(index, UINT64_MAX / 2);
    CHECK(child && smh_index_has_taxonomy(child));
    smh_index_free(child);
  } else {
    CHECK(smh_index_set_taxonomy(index, parent, 4, node_taxon, 3) != 0);   /* no index without a device */
    CHECK(smh_index_lca_many(index, queries, 2, coff, &taxa, &counts, qoff, per) == 2);
    CHECK(smh_index_lca_block_dev(index, NULL, off, 2, coff, &taxa, &counts, per, NULL) == 2);
    CHECK(smh_index_lca_sequences(index, rec, off, 2, rows) == 2);
    CHECK(smh_index_lca_sequences_dev(index, NULL, 0, off, 2, rows, NULL) == 2);
    CHECK(smh_index_lca_records(index, NULL, rows) == 2);
  }
  sourmash_err_clear();
  smh_index_free(index);
  for (int i = 0; i < 3; i++) kmerminhash_free(nodes[i]);
  kmerminhash_free(query);
  printf("lca abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
