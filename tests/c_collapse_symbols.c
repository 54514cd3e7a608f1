/* Link check of collapsing an index by groups and of the read-back (include/sourmash_amd.h, "Collapsing an index by groups"):
 * each entry point is called with the header's prototype.  Needs no GPU: with one a four-node index is collapsed into two
 * groups through plain C and read back, without one the device calls return 2 (the collapse: NULL with 2 in the error slot);
 * the geometry and the refusals of the arguments need no device either way. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(void) {
  uint32_t lane_max = 0, wave_max = 0, tile = 0;
  smh_collapse_geometry(&lane_max, &wave_max, &tile);
  CHECK(lane_max > 0 && wave_max > lane_max && tile > 0);
  smh_collapse_geometry(NULL, NULL, NULL);
  CHECK(SMH_COLLAPSE_FLAT == 0 && SMH_COLLAPSE_SUM == 1 && SMH_COLLAPSE_COUNT == 2 && SMH_COLLAPSE_DROP == 0xffffffffu);

  /* nodes {1, 2, 3, 4}, {3, 4, 5}, {5, 6}, {9}, every hash with abundance 2; groups {0, 1} and {2}, node 3 dropped */
  const int have = smh_device_available();
  const uint64_t held[4][4] = {{1, 2, 3, 4}, {3, 4, 5, 0}, {5, 6, 0, 0}, {9, 0, 0, 0}};
  KmerMinHash *nodes[4];
  for (int i = 0; i < 4; i++) {
    CHECK((nodes[i] = kmerminhash_new(0, 21, false, 42, UINT64_MAX, true)) != NULL);
    for (int k = 0; k < 4; k++)
      if (held[i][k]) { kmerminhash_add_hash(nodes[i], held[i][k]); kmerminhash_add_hash(nodes[i], held[i][k]); }
  }
  SmhIndex *index = smh_index_new(nodes, 4);
  CHECK((index != NULL) == (have != 0));
  sourmash_err_clear();
  const uint32_t group[4] = {0, 0, 1, SMH_COLLAPSE_DROP};

  /* refused before the index or the device is looked at */
  CHECK(smh_index_collapse(index, group, 0, 1, 0.0, SMH_COLLAPSE_FLAT) == NULL && sourmash_err_get_last_code() == 3);
  sourmash_err_clear();
  CHECK(smh_index_collapse(index, group, 2, 1, -0.5, SMH_COLLAPSE_FLAT) == NULL && sourmash_err_get_last_code() == 3);
  sourmash_err_clear();
  CHECK(smh_index_collapse(index, group, 2, 1, 1.5, SMH_COLLAPSE_FLAT) == NULL && sourmash_err_get_last_code() == 3);
  sourmash_err_clear();
  CHECK(smh_index_collapse(index, group, 2, 1, NAN, SMH_COLLAPSE_FLAT) == NULL && sourmash_err_get_last_code() == 3);
  sourmash_err_clear();
  CHECK(smh_index_collapse(index, group, 2, 1, 0.0, SMH_COLLAPSE_COUNT + 1) == NULL && sourmash_err_get_last_code() == 3);
  sourmash_err_clear();

  uint64_t off[5] = {77, 77, 77, 77, 77}, hashes[10] = {77, 77, 77, 77, 77, 77, 77, 77, 77, 77};
  uint32_t ab[10] = {77, 77, 77, 77, 77, 77, 77, 77, 77, 77};
  if (have) {
    /* a group beyond n_groups, a NULL index, NULL groups: MSG, nothing built */
    const uint32_t beyond[4] = {0, 2, 1, SMH_COLLAPSE_DROP};
    CHECK(smh_index_collapse(index, beyond, 2, 1, 0.0, SMH_COLLAPSE_FLAT) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    CHECK(smh_index_collapse(NULL, group, 2, 1, 0.0, SMH_COLLAPSE_FLAT) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    CHECK(smh_index_collapse(index, NULL, 2, 1, 0.0, SMH_COLLAPSE_FLAT) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();

    /* the union, with the abundances added up: {1, 2, 3, 4, 5} with 3 and 4 held twice, and {5, 6} */
    SmhIndex *u = smh_index_collapse(index, group, 2, 1, 0.0, SMH_COLLAPSE_SUM);
    CHECK(u != NULL && smh_index_len(u) == 2 && smh_index_has_abundances(u));
    CHECK(smh_index_read(u, off, hashes, ab) == 0);
    CHECK(off[0] == 0 && off[1] == 5 && off[2] == 7);
    const uint64_t want_h[7] = {1, 2, 3, 4, 5, 5, 6};
    const uint32_t want_a[7] = {2, 2, 4, 4, 2, 2, 2};
    for (int k = 0; k < 7; k++) CHECK(hashes[k] == want_h[k] && ab[k] == want_a[k]);
    CHECK(hashes[7] == 77 && ab[7] == 77);
    smh_index_free(u);
    /* the core, as a prevalence table: {3, 4} held by both members of group 0; group 1 has one member */
    SmhIndex *c = smh_index_collapse(index, group, 2, 1, 1.0, SMH_COLLAPSE_COUNT);
    CHECK(c != NULL && smh_index_read(c, off, hashes, ab) == 0);
    CHECK(off[1] == 2 && off[2] == 4 && hashes[0] == 3 && hashes[1] == 4 && hashes[2] == 5 && hashes[3] == 6);
    CHECK(ab[0] == 2 && ab[1] == 2 && ab[2] == 1 && ab[3] == 1);
    smh_index_free(c);
    /* flat: no abundances to read; every output of the read-back is nullable */
    SmhIndex *f = smh_index_collapse(index, group, 2, 2, 0.0, SMH_COLLAPSE_FLAT);
    CHECK(f != NULL && !smh_index_has_abundances(f));
    CHECK(smh_index_read(f, off, NULL, NULL) == 0 && off[1] == 2 && off[2] == 2);
    CHECK(smh_index_read(f, NULL, hashes, NULL) == 0 && hashes[0] == 3 && hashes[1] == 4);
    ab[0] = 77;
    CHECK(smh_index_read(f, NULL, NULL, ab) == 3 && ab[0] == 77);
    sourmash_err_clear();
    smh_index_free(f);
    /* the parent reads back as it was built */
    CHECK(smh_index_read(index, off, NULL, NULL) == 0 && off[0] == 0 && off[1] == 4 && off[2] == 7 && off[3] == 9 && off[4] == 10);
    CHECK(smh_index_read(index, NULL, hashes, ab) == 0 && hashes[4] == 3 && hashes[9] == 9 && ab[0] == 2 && ab[9] == 2);
  } else {
    CHECK(smh_index_collapse(index, group, 2, 1, 0.0, SMH_COLLAPSE_FLAT) == NULL && sourmash_err_get_last_code() == 2);
    sourmash_err_clear();
    CHECK(smh_index_read(index, off, hashes, ab) == 2);
    CHECK(off[0] == 77 && hashes[0] == 77 && ab[0] == 77);
  }
  sourmash_err_clear();
  smh_index_free(index);
  for (int i = 0; i < 4; i++) kmerminhash_free(nodes[i]);
  printf("collapse abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
