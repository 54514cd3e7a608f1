/* Link check of building an index from records and of concatenation (include/sourmash_amd.h, "Building an index from
 * records"): each entry point is called with the header's prototype.  Needs no GPU: every refusal of the arguments is MSG (3)
 * with or without one -- it comes before the device is touched -- and a valid call without a device returns NULL with 2 in
 * the error slot.  With a GPU three records are built into two nodes through plain C, compared with sketches filled by
 * kmerminhash_add_sequence, and concatenated. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
#define REFUSED(call) do { sourmash_err_clear(); CHECK((call) == NULL && sourmash_err_get_last_code() == 3); sourmash_err_clear(); } while (0)

int main(void) {
  uint32_t tile = 0, threads = 0;
  smh_index_build_geometry(&tile, &threads);
  CHECK(tile > 0 && threads > 0 && tile % threads == 0);
  smh_index_build_geometry(NULL, NULL);
  CHECK(SMH_INPUT_NUCLEOTIDE == 0 && SMH_INPUT_AMINO == 1);
  const uint64_t budget = smh_index_build_budget();
  CHECK(budget > 0);
  smh_index_build_set_budget(150);
  CHECK(smh_index_build_budget() == 150);
  smh_index_build_set_budget(0);
  CHECK(smh_index_build_budget() == budget);

  const int have = smh_device_available();
  /* three records: groups 0, 1, 0 */
  const char *seq = "ACGTTGCAAGGCTTAACCGGTTAGCATCGATCGGATCAAGGCTTAACCGGTTAGCATCGATNGATTACAGATTACAGATTACAGGATCC";
  const uint64_t off[4] = {0, 30, 61, (uint64_t)strlen(seq)};
  const uint32_t groups[3] = {0, 1, 0};
  KmerMinHash *like = kmerminhash_new(0, 21, false, 42, UINT64_MAX, true);
  KmerMinHash *num_like = kmerminhash_new(500, 21, false, 42, 0, false);
  KmerMinHash *k0_like = kmerminhash_new(0, 0, false, 42, UINT64_MAX, false);
  KmerMinHash *prot_like = kmerminhash_new(0, 21, true, 42, UINT64_MAX, false);
  KmerMinHash *prot_k2 = kmerminhash_new(0, 2, true, 42, UINT64_MAX, false);
  CHECK(like && num_like && k0_like && prot_like && prot_k2);

  /* the refusals of the arguments: MSG, before the device is touched */
  REFUSED(smh_index_from_sequences(NULL, SMH_INPUT_NUCLEOTIDE, seq, off, groups, 3, 2));
  REFUSED(smh_index_from_sequences(like, SMH_INPUT_NUCLEOTIDE, seq, NULL, groups, 3, 2));
  REFUSED(smh_index_from_sequences(like, SMH_INPUT_NUCLEOTIDE, NULL, off, groups, 3, 2));
  REFUSED(smh_index_from_sequences(like, 2, seq, off, groups, 3, 2));
  REFUSED(smh_index_from_sequences(num_like, SMH_INPUT_NUCLEOTIDE, seq, off, groups, 3, 2));
  REFUSED(smh_index_from_sequences(like, SMH_INPUT_AMINO, seq, off, groups, 3, 2));
  const uint64_t descending[4] = {0, 40, 30, 88};
  REFUSED(smh_index_from_sequences(like, SMH_INPUT_NUCLEOTIDE, seq, descending, groups, 3, 2));
  REFUSED(smh_index_from_sequences_dev(like, SMH_INPUT_NUCLEOTIDE, (const void *)seq, 50, off, groups, 3, 2, NULL));   /* beyond total_len */
  const uint32_t beyond[3] = {0, 2, 0};
  REFUSED(smh_index_from_sequences(like, SMH_INPUT_NUCLEOTIDE, seq, off, beyond, 3, 2));
  REFUSED(smh_index_from_sequences(like, SMH_INPUT_NUCLEOTIDE, seq, off, NULL, 3, 2));
  REFUSED(smh_index_from_sequences(k0_like, SMH_INPUT_NUCLEOTIDE, seq, off, groups, 3, 2));
  REFUSED(smh_index_from_sequences(prot_k2, SMH_INPUT_NUCLEOTIDE, seq, off, groups, 3, 2));
  REFUSED(smh_index_from_sequences(prot_k2, SMH_INPUT_AMINO, seq, off, groups, 3, 2));
  REFUSED(smh_index_from_sequences(like, SMH_INPUT_NUCLEOTIDE, seq, off, groups, 3, 1u << 24));
  REFUSED(smh_index_from_records(like, SMH_INPUT_NUCLEOTIDE, NULL, groups, 2));
  REFUSED(smh_index_concat(NULL, 2));
  SmhIndex *holes[2] = {NULL, NULL};
  REFUSED(smh_index_concat(holes, 2));

  if (!have) {
    sourmash_err_clear();
    CHECK(smh_index_from_sequences(like, SMH_INPUT_NUCLEOTIDE, seq, off, groups, 3, 2) == NULL && sourmash_err_get_last_code() == 2);
    sourmash_err_clear();
    CHECK(smh_index_from_sequences_dev(like, SMH_INPUT_NUCLEOTIDE, (const void *)seq, off[3], off, NULL, 3, 3, NULL) == NULL &&
          sourmash_err_get_last_code() == 2);
    sourmash_err_clear();
    CHECK(smh_index_from_sequences(prot_like, SMH_INPUT_AMINO, seq, off, groups, 3, 2) == NULL && sourmash_err_get_last_code() == 2);
    sourmash_err_clear();
    CHECK(smh_index_concat(NULL, 0) == NULL && sourmash_err_get_last_code() == 2);
    sourmash_err_clear();
  } else {
    SmhIndex *built = smh_index_from_sequences(like, SMH_INPUT_NUCLEOTIDE, seq, off, groups, 3, 2);
    CHECK(built != NULL && smh_index_len(built) == 2 && smh_index_has_abundances(built) && smh_index_all_scaled(built));
    /* the witnesses: fresh sketches of like's parameters, filled record by record */
    KmerMinHash *want[2];
    char rec[64];
    for (int g = 0; g < 2; g++) CHECK((want[g] = kmerminhash_new(0, 21, false, 42, UINT64_MAX, true)) != NULL);
    for (int r = 0; r < 3; r++) {
      const size_t len = (size_t)(off[r + 1] - off[r]);
      memcpy(rec, seq + off[r], len);
      rec[len] = 0;
      kmerminhash_add_sequence(want[groups[r]], rec, true);
    }
    uint64_t o[3] = {77, 77, 77}, hashes[128];
    uint32_t ab[128];
    CHECK(smh_index_read(built, o, hashes, ab) == 0 && o[0] == 0);
    for (int g = 0; g < 2; g++) {
      const size_t n = kmerminhash_get_mins_size(want[g]);
      CHECK(o[g + 1] - o[g] == n && n > 0);
      for (size_t k = 0; k < n; k++)
        CHECK(hashes[o[g] + k] == kmerminhash_get_min_idx(want[g], k) && ab[o[g] + k] == kmerminhash_get_abund_idx(want[g], k));
    }
    /* one node per record without group ids, through the device-pointer form is left to the Python tests; concat here */
    SmhIndex *parts[2] = {built, built};
    SmhIndex *twice = smh_index_concat(parts, 2);
    CHECK(twice != NULL && smh_index_len(twice) == 4 && smh_index_has_abundances(twice));
    smh_index_free(built);   /* the result owns its memory */
    uint64_t o2[5], h2[256];
    CHECK(smh_index_read(twice, o2, h2, NULL) == 0 && o2[4] == 2 * o[2] && o2[2] == o[2]);
    for (uint64_t k = 0; k < o[2]; k++) CHECK(h2[k] == hashes[k] && h2[o[2] + k] == hashes[k]);
    smh_index_free(twice);
    SmhIndex *none = smh_index_concat(NULL, 0);
    CHECK(none != NULL && smh_index_len(none) == 0);
    smh_index_free(none);
    for (int g = 0; g < 2; g++) kmerminhash_free(want[g]);
  }
  kmerminhash_free(like); kmerminhash_free(num_like); kmerminhash_free(k0_like); kmerminhash_free(prot_like); kmerminhash_free(prot_k2);
  printf("index build abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
