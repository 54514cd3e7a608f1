/* Link check of the entry points that gather a batch of queries (include/sourmash_amd.h, smh_index_gather_many): each is
 * called with the header's prototype, and the rows are freed with free().  Needs no GPU: with one the batch answers as two
 * single calls do, without one every device call returns 2; the budget needs no device either way. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static KmerMinHash *sketch(const uint64_t *h, int n) {
  KmerMinHash *mh = kmerminhash_new(0, 21, false, 42, UINT64_MAX, false);
  for (int i = 0; mh && i < n; i++) kmerminhash_add_hash(mh, h[i]);
  return mh;
}

int main(void) {
  const uint64_t def = smh_gather_many_budget();
  CHECK(def == (1ull << 26));
  smh_gather_many_set_budget(12345);
  CHECK(smh_gather_many_budget() == 12345);
  smh_gather_many_set_budget(0);
  CHECK(smh_gather_many_budget() == def);

  const int have = smh_device_available();
  const uint64_t a[3] = {1, 2, 3}, b[2] = {3, 4}, q0[4] = {1, 2, 3, 4}, q1[2] = {4, 9};
  KmerMinHash *nodes[2] = {sketch(a, 3), sketch(b, 2)};
  KmerMinHash *qs[2] = {sketch(q0, 4), sketch(q1, 2)};
  CHECK(nodes[0] && nodes[1] && qs[0] && qs[1]);
  SmhIndex *index = smh_index_new(nodes, 2);
  CHECK((index != NULL) == (have != 0));
  sourmash_err_clear();

  const KmerMinHash *const batch[2] = {qs[0], qs[1]};
  uint64_t row_off[3] = {9, 9, 9}, q_off[3] = {9, 9, 9};
  uint32_t assigned[6];
  SmhGatherRow *rows = NULL;
  const int rc = smh_index_gather_many(index, batch, 2, 0, 10, row_off, &rows, q_off, assigned);
  CHECK(rc == (have ? 0 : 2));
  if (have) {
    CHECK(rows && row_off[0] == 0 && row_off[1] == 2 && row_off[2] == 3);
    CHECK(q_off[0] == 0 && q_off[1] == 4 && q_off[2] == 6);
    CHECK(rows[0].match == 0 && rows[0].common_remaining == 3 && rows[0].size_match == 3 && rows[0].abund_sum == 3);
    CHECK(rows[1].match == 1 && rows[1].common_remaining == 1 && rows[1].common_original == 2);
    CHECK(rows[2].match == 1 && rows[2].common_remaining == 1 && rows[2].common_original == 1);
    CHECK(assigned[0] == 0 && assigned[2] == 0 && assigned[3] == 1 && assigned[4] == 0 && assigned[5] == 0xffffffffu);
    /* the single-query route says the same */
    SmhGatherRow one[2];
    uint32_t n_one = 0;
    CHECK(smh_index_gather(index, qs[0], 0, one, 2, &n_one, NULL) == 0 && n_one == 2);
    CHECK(memcmp(one, rows, sizeof one) == 0);
    free(rows);
    /* the device form with an empty batch: zero rows, one element allocated */
    const uint64_t none[1] = {0};
    uint64_t roff[1] = {9};
    rows = NULL;
    CHECK(smh_index_gather_block_dev(index, NULL, NULL, none, 0, 1, 10, roff, &rows, NULL, NULL) == 0);
    CHECK(rows && roff[0] == 0);
    free(rows);
  } else {
    CHECK(rows == NULL && row_off[0] == 9 && q_off[2] == 9);
    const uint64_t none[1] = {0};
    CHECK(smh_index_gather_block_dev(index, NULL, NULL, none, 0, 1, 10, row_off, &rows, NULL, NULL) == 2);
    CHECK(rows == NULL);
  }
  sourmash_err_clear();
  smh_index_free(index);
  for (int i = 0; i < 2; i++) { kmerminhash_free(nodes[i]); kmerminhash_free(qs[i]); }
  printf("gather many abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
