/* Link check of filtering an index and of taking a subset of its nodes (include/sourmash_amd.h, "Filtering an index"): each
 * entry point is called with the header's prototype.  Needs no GPU: with one a four-node index is filtered and selected
 * through plain C and read back, without one the device calls return NULL with 2 in the error slot; the geometry and the
 * refusals of the rule alone need no device either way. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(void) {
  uint32_t tile = 0, samples = 0, threads = 0;
  smh_filter_geometry(&tile, &samples, &threads);
  CHECK(tile >= 64 && tile % 64 == 0 && samples > 1 && threads >= 64 && threads % 64 == 0);
  smh_filter_geometry(NULL, NULL, NULL);
  CHECK(SMH_FILTER_OPERAND_NONE == 0 && SMH_FILTER_KEEP_IN == 1 && SMH_FILTER_DROP_IN == 2);
  CHECK(SMH_FILTER_ABUND_OWN == 0 && SMH_FILTER_ABUND_FLAT == 1 && SMH_FILTER_ABUND_OPERAND == 2);
  CHECK(sizeof(SmhFilter) == 24);

  /* nodes {1, 2, 3, 4}, {3, 4, 5}, {5, 6}, {9}, every hash with abundance 2; the operand {2, 3, 5, 7} with abundance 3 */
  const int have = smh_device_available();
  const uint64_t held[4][4] = {{1, 2, 3, 4}, {3, 4, 5, 0}, {5, 6, 0, 0}, {9, 0, 0, 0}};
  const uint64_t op_held[4] = {2, 3, 5, 7};
  KmerMinHash *nodes[4];
  for (int i = 0; i < 4; i++) {
    CHECK((nodes[i] = kmerminhash_new(0, 21, false, 42, UINT64_MAX, true)) != NULL);
    for (int k = 0; k < 4; k++)
      if (held[i][k]) { kmerminhash_add_hash(nodes[i], held[i][k]); kmerminhash_add_hash(nodes[i], held[i][k]); }
  }
  KmerMinHash *operand = kmerminhash_new(0, 21, false, 42, UINT64_MAX, true);
  CHECK(operand != NULL);
  for (int k = 0; k < 4; k++)
    for (int r = 0; r < 3; r++) kmerminhash_add_hash(operand, op_held[k]);
  SmhIndex *index = smh_index_new(nodes, 4);
  CHECK((index != NULL) == (have != 0));
  sourmash_err_clear();

  /* the rule's own refusals come before the index or the device is looked at */
  SmhFilter rule = {SMH_FILTER_OPERAND_NONE, SMH_FILTER_ABUND_OWN, 0, 0xffffffffu, 0, 0xffffffffu};
  CHECK(smh_index_filter(index, NULL, NULL) == NULL && sourmash_err_get_last_code() == 3);
  sourmash_err_clear();
  rule.operand_mode = 3;
  CHECK(smh_index_filter(index, operand, &rule) == NULL && sourmash_err_get_last_code() == 3);
  sourmash_err_clear();
  rule.operand_mode = SMH_FILTER_OPERAND_NONE; rule.abund_out = 3;
  CHECK(smh_index_filter(index, operand, &rule) == NULL && sourmash_err_get_last_code() == 3);
  sourmash_err_clear();
  rule.abund_out = SMH_FILTER_ABUND_OWN; rule.min_abund = 2; rule.max_abund = 1;
  CHECK(smh_index_filter(index, operand, &rule) == NULL && sourmash_err_get_last_code() == 3);
  sourmash_err_clear();
  rule.min_abund = 0; rule.max_abund = 0xffffffffu; rule.min_owners = 3; rule.max_owners = 2;
  CHECK(smh_index_filter(index, operand, &rule) == NULL && sourmash_err_get_last_code() == 3);
  sourmash_err_clear();
  rule.min_owners = 0; rule.max_owners = 0xffffffffu; rule.operand_mode = SMH_FILTER_DROP_IN; rule.abund_out = SMH_FILTER_ABUND_OPERAND;
  CHECK(smh_index_filter(index, operand, &rule) == NULL && sourmash_err_get_last_code() == 3);
  sourmash_err_clear();

  uint64_t off[6] = {77, 77, 77, 77, 77, 77}, hashes[12];
  uint32_t ab[12];
  for (int k = 0; k < 12; k++) { hashes[k] = 77; ab[k] = 77; }
  const uint32_t ids[3] = {3, 1, 1};
  if (have) {
    /* a NULL index, a missing operand, an id beyond the nodes: MSG, nothing built */
    rule.operand_mode = SMH_FILTER_KEEP_IN; rule.abund_out = SMH_FILTER_ABUND_OWN;
    CHECK(smh_index_filter(NULL, operand, &rule) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    CHECK(smh_index_filter(index, NULL, &rule) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    const uint32_t beyond[2] = {0, 4};
    CHECK(smh_index_select(index, beyond, 2) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    CHECK(smh_index_select(NULL, ids, 3) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();

    /* intersect: {2, 3}, {3, 5}, {5}, {} with the nodes' own abundances */
    SmhIndex *k = smh_index_filter(index, operand, &rule);
    CHECK(k != NULL && smh_index_len(k) == 4 && smh_index_has_abundances(k));
    CHECK(smh_index_read(k, off, hashes, ab) == 0);
    CHECK(off[0] == 0 && off[1] == 2 && off[2] == 4 && off[3] == 5 && off[4] == 5);
    const uint64_t want_k[5] = {2, 3, 3, 5, 5};
    for (int i = 0; i < 5; i++) CHECK(hashes[i] == want_k[i] && ab[i] == 2);
    CHECK(hashes[5] == 77 && ab[5] == 77);
    smh_index_free(k);
    /* inflate: the same hashes with the operand's abundances */
    rule.abund_out = SMH_FILTER_ABUND_OPERAND;
    SmhIndex *inf = smh_index_filter(index, operand, &rule);
    CHECK(inf != NULL && smh_index_read(inf, off, hashes, ab) == 0 && off[4] == 5);
    for (int i = 0; i < 5; i++) CHECK(hashes[i] == want_k[i] && ab[i] == 3);
    smh_index_free(inf);
    /* subtract, flattened: {1, 4}, {4}, {6}, {9} */
    rule.operand_mode = SMH_FILTER_DROP_IN; rule.abund_out = SMH_FILTER_ABUND_FLAT;
    SmhIndex *d = smh_index_filter(index, operand, &rule);
    CHECK(d != NULL && !smh_index_has_abundances(d) && smh_index_read(d, off, hashes, NULL) == 0);
    CHECK(off[1] == 2 && off[2] == 3 && off[3] == 4 && off[4] == 5);
    CHECK(hashes[0] == 1 && hashes[1] == 4 && hashes[2] == 4 && hashes[3] == 6 && hashes[4] == 9);
    smh_index_free(d);
    /* the private hashes, no operand: {1, 2}, {}, {6}, {9} */
    SmhFilter own = {SMH_FILTER_OPERAND_NONE, SMH_FILTER_ABUND_OWN, 0, 0xffffffffu, 1, 1};
    SmhIndex *p = smh_index_filter(index, NULL, &own);
    CHECK(p != NULL && smh_index_read(p, off, hashes, ab) == 0);
    CHECK(off[1] == 2 && off[2] == 2 && off[3] == 3 && off[4] == 4 && hashes[0] == 1 && hashes[1] == 2 && hashes[2] == 6 && hashes[3] == 9);
    smh_index_free(p);
    /* select: nodes 3, 1, 1 */
    SmhIndex *sel = smh_index_select(index, ids, 3);
    CHECK(sel != NULL && smh_index_len(sel) == 3 && smh_index_read(sel, off, hashes, ab) == 0);
    CHECK(off[0] == 0 && off[1] == 1 && off[2] == 4 && off[3] == 7);
    const uint64_t want_s[7] = {9, 3, 4, 5, 3, 4, 5};
    for (int i = 0; i < 7; i++) CHECK(hashes[i] == want_s[i] && ab[i] == 2);
    smh_index_free(sel);
    SmhIndex *none = smh_index_select(index, NULL, 0);
    CHECK(none != NULL && smh_index_len(none) == 0);
    smh_index_free(none);
    /* the parent reads back as it was built */
    CHECK(smh_index_read(index, off, NULL, NULL) == 0 && off[0] == 0 && off[1] == 4 && off[2] == 7 && off[3] == 9 && off[4] == 10);
  } else {
    rule.operand_mode = SMH_FILTER_KEEP_IN; rule.abund_out = SMH_FILTER_ABUND_OWN;
    CHECK(smh_index_filter(index, operand, &rule) == NULL && sourmash_err_get_last_code() == 2);
    sourmash_err_clear();
    CHECK(smh_index_select(index, ids, 3) == NULL && sourmash_err_get_last_code() == 2);
  }
  sourmash_err_clear();
  smh_index_free(index);
  kmerminhash_free(operand);
  for (int i = 0; i < 4; i++) kmerminhash_free(nodes[i]);
  printf("filter abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
