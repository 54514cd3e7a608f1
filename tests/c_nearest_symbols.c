/* Link check of the nearest-neighbour entry points (include/sourmash_amd.h, smh_index_nearest_many): each is called with the
 * header's prototype.  Needs no GPU: with one a four-node index answers through plain C, without one every device call
 * returns 2; the geometry and the refusals of k, a NaN threshold and an unknown metric need no device either way. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(void) {
  uint32_t max_k = 0, tile = 0, slots = 0, search_tile = 0;
  smh_nearest_geometry(&max_k, &tile, &slots);
  smh_search_geometry(NULL, &search_tile, NULL);
  CHECK(max_k >= 100 && tile == search_tile && slots >= tile && slots > max_k && (slots & (slots - 1)) == 0);
  smh_nearest_geometry(NULL, NULL, NULL);

  /* nodes {1, 2}, {1, 2, 3, 4}, {9}, {2, 5}; queries {1}, {}, {1, 2, 3, 4} */
  const int have = smh_device_available();
  KmerMinHash *nodes[4], *qs[3];
  for (int i = 0; i < 4; i++) CHECK((nodes[i] = kmerminhash_new(0, 21, false, 42, UINT64_MAX, false)) != NULL);
  for (int i = 0; i < 3; i++) CHECK((qs[i] = kmerminhash_new(0, 21, false, 42, UINT64_MAX, false)) != NULL);
  for (uint64_t h = 1; h <= 4; h++) {
    if (h <= 2) kmerminhash_add_hash(nodes[0], h);
    kmerminhash_add_hash(nodes[1], h);
    kmerminhash_add_hash(qs[2], h);
  }
  kmerminhash_add_hash(nodes[2], 9);
  kmerminhash_add_hash(nodes[3], 2);
  kmerminhash_add_hash(nodes[3], 5);
  kmerminhash_add_hash(qs[0], 1);
  SmhIndex *index = smh_index_new(nodes, 4);
  CHECK((index != NULL) == (have != 0));
  sourmash_err_clear();

  const KmerMinHash *queries[3] = {qs[0], qs[1], qs[2]};
  uint64_t roff[5] = {9, 9, 9, 9, 9};
  SmhSearchRow *rows = NULL;
  /* refused before the index or the device is looked at; nothing written */
  CHECK(smh_index_nearest_many(index, queries, 3, 0, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows) == 3);
  CHECK(smh_index_nearest_many(index, queries, 3, max_k + 1, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows) == 3);
  CHECK(smh_index_nearest_self(index, 0, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows) == 3);
  CHECK(smh_index_nearest_self(index, max_k + 1, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows) == 3);
  CHECK(smh_index_nearest_block_dev(index, NULL, roff, 0, 0, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows, NULL) == 3);
  CHECK(smh_index_nearest_block_dev(index, NULL, roff, 0, UINT32_MAX, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows, NULL) == 3);
  CHECK(smh_index_nearest_many(index, queries, 3, 1, SMH_SEARCH_JACCARD, NAN, 0, roff, &rows) == 3);
  CHECK(smh_index_nearest_many(index, queries, 3, 1, 4, 0.1, 0, roff, &rows) == 3);
  CHECK(smh_index_nearest_self(index, 1, SMH_SEARCH_MAX_CONTAINMENT + 1, 0.1, 0, roff, &rows) == 3);
  CHECK(smh_index_nearest_block_dev(index, NULL, roff, 0, 1, SMH_SEARCH_JACCARD, NAN, 0, roff, &rows, NULL) == 3);
  CHECK(smh_index_nearest_many(index, queries, 3, 1, SMH_SEARCH_JACCARD, 0.1, 0, NULL, &rows) == 1);
  CHECK(smh_index_nearest_self(index, 1, SMH_SEARCH_JACCARD, 0.1, 0, roff, NULL) == 1);
  CHECK(roff[0] == 9 && roff[4] == 9 && rows == NULL);
  sourmash_err_clear();

  if (have) {
    /* CONTAINMENT_NODE, k = 2: query {1} has 1/2 at node 0 and 1/4 at node 1; query {1, 2, 3, 4} has 1.0 at nodes 0 and 1
     * (the lower node first) and 1/2 at node 3, which k cuts off */
    CHECK(smh_index_nearest_many(index, queries, 3, 2, SMH_SEARCH_CONTAINMENT_NODE, 0.0, 0, roff, &rows) == 0);
    CHECK(roff[0] == 0 && roff[1] == 2 && roff[2] == 2 && roff[3] == 4);
    CHECK(rows[0].node == 0 && rows[0].common == 1 && rows[0].node_size == 2 && rows[0].query_size == 1);
    CHECK(rows[1].node == 1 && rows[1].common == 1 && rows[1].node_size == 4);
    CHECK(rows[2].node == 0 && rows[2].common == 2 && rows[2].query_size == 4 && rows[3].node == 1 && rows[3].common == 4);
    free(rows); rows = NULL;
    /* JACCARD, k = 1: the query {1, 2, 3, 4} IS node 1 */
    CHECK(smh_index_nearest_many(index, queries, 3, 1, SMH_SEARCH_JACCARD, 0.0, 0, roff, &rows) == 0);
    CHECK(roff[1] == 1 && roff[3] == 2 && rows[0].node == 0 && rows[1].node == 1 && rows[1].common == 4 && rows[1].node_size == 4);
    free(rows); rows = NULL;
    /* the index against itself, k = 1: node 0 -> 1 (2/4), node 1 -> 0, node 2 -> nobody, node 3 -> 0 (1/3, not 1 at 1/5) */
    CHECK(smh_index_nearest_self(index, 1, SMH_SEARCH_JACCARD, 0.0, 0, roff, &rows) == 0);
    CHECK(roff[0] == 0 && roff[1] == 1 && roff[2] == 2 && roff[3] == 2 && roff[4] == 3);
    CHECK(rows[0].node == 1 && rows[0].common == 2 && rows[1].node == 0 && rows[2].node == 0 && rows[2].common == 1);
    free(rows); rows = NULL;
    CHECK(smh_index_nearest_self(index, 3, SMH_SEARCH_JACCARD, 0.9, 0, roff, &rows) == 0);
    CHECK(roff[4] == 0 && rows != NULL);   /* one element at least is allocated */
    free(rows); rows = NULL;
    /* the CSR form on hashes that already live in device memory: parsed records' bytes serve as one 8-byte "hash" nobody holds */
    SmhRecords *parsed = smh_records_parse(">a\nCTCGAATAAAAGTAGACTTCACGCCCTTAA\n", 34, 0);
    CHECK(parsed != NULL);
    const uint64_t boff[2] = {0, 1};
    CHECK(smh_index_nearest_block_dev(index, (const uint64_t *)smh_records_seq_dev(parsed), boff, 1, 5, SMH_SEARCH_CONTAINMENT_QUERY, 0.0, 0,
                                      roff, &rows, NULL) == 0);
    CHECK(roff[0] == 0 && roff[1] == 0);
    free(rows); rows = NULL;
    smh_records_free(parsed);
    KmerMinHash *num = kmerminhash_new(5, 21, false, 42, 0, false);
    const KmerMinHash *bad[2] = {qs[0], num};
    roff[0] = 9;
    CHECK(smh_index_nearest_many(index, bad, 2, 1, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows) == 3);
    CHECK(roff[0] == 9 && rows == NULL);
    kmerminhash_free(num);
  } else {
    CHECK(smh_index_nearest_many(index, queries, 3, 1, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows) == 2);
    CHECK(smh_index_nearest_block_dev(index, NULL, roff, 0, 1, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows, NULL) == 2);
    CHECK(smh_index_nearest_self(index, 1, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows) == 2);
    CHECK(rows == NULL);
  }
  sourmash_err_clear();
  smh_index_free(index);
  for (int i = 0; i < 4; i++) kmerminhash_free(nodes[i]);
  for (int i = 0; i < 3; i++) kmerminhash_free(qs[i]);
  printf("nearest abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
