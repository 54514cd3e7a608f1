/* Link check of the batch search entry points (include/sourmash_amd.h, smh_index_search_many): each is called with the
 * header's prototype.  Needs no GPU: with one a three-node index answers through plain C, without one every device call
 * returns 2; the geometry, the budget and the refusals of a NaN threshold and an unknown metric need no device either way. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(void) {
  uint32_t short_owners = 0, tile = 0, max_queries = 0;
  smh_search_geometry(&short_owners, &tile, &max_queries);
  CHECK(short_owners > 0 && tile >= 64 && tile % 64 == 0 && max_queries == 65535);
  const uint64_t def = smh_search_many_budget();
  CHECK(def == (1ull << 26));
  smh_search_many_set_budget(12345);
  CHECK(smh_search_many_budget() == 12345);
  smh_search_many_set_budget(0);
  CHECK(smh_search_many_budget() == def);
  CHECK(sizeof(SmhSearchRow) == 16);

  /* nodes {1, 2}, {1, 2, 3, 4}, {9}; queries {1}, {}, {1, 2, 3, 4} */
  const int have = smh_device_available();
  KmerMinHash *nodes[3], *qs[3];
  for (int i = 0; i < 3; i++) {
    CHECK((nodes[i] = kmerminhash_new(0, 21, false, 42, UINT64_MAX, false)) != NULL);
    CHECK((qs[i] = kmerminhash_new(0, 21, false, 42, UINT64_MAX, false)) != NULL);
  }
  for (uint64_t h = 1; h <= 4; h++) {
    if (h <= 2) kmerminhash_add_hash(nodes[0], h);
    kmerminhash_add_hash(nodes[1], h);
    kmerminhash_add_hash(qs[2], h);
  }
  kmerminhash_add_hash(nodes[2], 9);
  kmerminhash_add_hash(qs[0], 1);
  SmhIndex *index = smh_index_new(nodes, 3);
  CHECK((index != NULL) == (have != 0));
  sourmash_err_clear();

  const KmerMinHash *queries[3] = {qs[0], qs[1], qs[2]};
  uint64_t roff[4] = {9, 9, 9, 9};
  SmhSearchRow *rows = NULL;
  /* refused before the index or the device is looked at; nothing written */
  CHECK(smh_index_search_many(index, queries, 3, SMH_SEARCH_JACCARD, NAN, 0, roff, &rows) == 3);
  CHECK(smh_index_search_many(index, queries, 3, 4, 0.1, 0, roff, &rows) == 3);
  CHECK(smh_index_search_self(index, SMH_SEARCH_MAX_CONTAINMENT + 1, 0.1, 0, true, roff, &rows) == 3);
  CHECK(smh_index_search_block_dev(index, NULL, roff, 0, SMH_SEARCH_JACCARD, NAN, 0, roff, &rows, NULL) == 3);
  CHECK(smh_index_search_many(index, queries, 3, SMH_SEARCH_JACCARD, 0.1, 0, NULL, &rows) == 1);
  CHECK(smh_index_search_self(index, SMH_SEARCH_JACCARD, 0.1, 0, false, roff, NULL) == 1);
  CHECK(roff[0] == 9 && roff[3] == 9 && rows == NULL);
  sourmash_err_clear();

  if (have) {
    /* CONTAINMENT_NODE > 0.25: query {1} reaches node 0 (1 / 2) and not node 1 (1 / 4: the comparison is strict) */
    CHECK(smh_index_search_many(index, queries, 3, SMH_SEARCH_CONTAINMENT_NODE, 0.25, 0, roff, &rows) == 0);
    CHECK(roff[0] == 0 && roff[1] == 1 && roff[2] == 1 && roff[3] == 3);
    CHECK(rows[0].node == 0 && rows[0].common == 1 && rows[0].node_size == 2 && rows[0].query_size == 1);
    CHECK(rows[1].node == 0 && rows[1].common == 2 && rows[1].query_size == 4 && rows[2].node == 1 && rows[2].common == 4);
    free(rows); rows = NULL;
    /* the index against itself: nodes 0 and 1 share two hashes; jaccard 2 / 4 */
    CHECK(smh_index_search_self(index, SMH_SEARCH_JACCARD, 0.4, 0, true, roff, &rows) == 0);
    CHECK(roff[0] == 0 && roff[1] == 1 && roff[2] == 1 && roff[3] == 1 && rows[0].node == 1 && rows[0].common == 2);
    free(rows); rows = NULL;
    CHECK(smh_index_search_self(index, SMH_SEARCH_JACCARD, 0.5, 0, false, roff, &rows) == 0);
    CHECK(roff[3] == 0 && rows != NULL);   /* one element at least is allocated */
    free(rows); rows = NULL;
    /* the CSR form on hashes that already live in device memory: parsed records' bytes serve as one 8-byte "hash" nobody holds */
    SmhRecords *parsed = smh_records_parse(">a\nCTCGAATAAAAGTAGACTTCACGCCCTTAA\n", 34, 0);
    CHECK(parsed != NULL);
    const uint64_t boff[2] = {0, 1};
    CHECK(smh_index_search_block_dev(index, (const uint64_t *)smh_records_seq_dev(parsed), boff, 1, SMH_SEARCH_CONTAINMENT_QUERY, 0.0, 0,
                                     roff, &rows, NULL) == 0);
    CHECK(roff[0] == 0 && roff[1] == 0);
    free(rows); rows = NULL;
    smh_records_free(parsed);
    KmerMinHash *num = kmerminhash_new(5, 21, false, 42, 0, false);
    const KmerMinHash *bad[2] = {qs[0], num};
    roff[0] = 9;
    CHECK(smh_index_search_many(index, bad, 2, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows) == 3);
    CHECK(roff[0] == 9 && rows == NULL);
    kmerminhash_free(num);
  } else {
    CHECK(smh_index_search_many(index, queries, 3, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows) == 2);
    CHECK(smh_index_search_block_dev(index, NULL, roff, 0, SMH_SEARCH_JACCARD, 0.1, 0, roff, &rows, NULL) == 2);
    CHECK(smh_index_search_self(index, SMH_SEARCH_JACCARD, 0.1, 0, true, roff, &rows) == 2);
    CHECK(rows == NULL);
  }
  sourmash_err_clear();
  smh_index_free(index);
  for (int i = 0; i < 3; i++) { kmerminhash_free(nodes[i]); kmerminhash_free(qs[i]); }
  printf("search_many abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
