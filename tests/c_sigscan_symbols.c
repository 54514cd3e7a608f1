/* Link check of signature JSON read on the device (include/sourmash_amd.h, "Signature JSON on the device"): each entry point is
 * called with the header's prototype.  Needs no GPU: with one a document of two sketches is parsed from plain C, its entries,
 * spans and index are read back and every refusal is met; without one the device calls return NULL with 2 in the error slot
 * and the accessors answer for a NULL handle. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static const char *DOC =
    "[{\"class\":\"sourmash_signature\",\"email\":\"\",\"hash_function\":\"0.murmur64\",\"filename\":null,\"name\":\"a [1,2] name\","
    "\"license\":\"CC0\",\"signatures\":["
    "{\"num\":0,\"ksize\":21,\"seed\":42,\"max_hash\":1000,\"mins\":[3, 5,\n9],\"md5sum\":\"abc\",\"abundances\":[1,2,4294967296],\"molecule\":\"DNA\"},"
    "{\"num\":500,\"ksize\":31,\"seed\":42,\"max_hash\":0,\"mins\":[7,8],\"md5sum\":\"def\",\"molecule\":\"protein\"}],\"version\":0.4}]";

int main(void) {
  uint32_t tile = 0, threads = 0;
  smh_sigscan_geometry(&tile, &threads);
  CHECK(tile >= 256 && tile % 16 == 0 && threads >= 64 && threads % 64 == 0);
  smh_sigscan_geometry(NULL, NULL);
  CHECK(SMH_SIGSPAN_CLOSED == 0 && SMH_SIGSPAN_OPEN == 1 && SMH_SIGSPAN_OVERFLOW == 2 && SMH_SIGSPAN_BAD_SYNTAX == 3);
  /* a NULL handle */
  CHECK(smh_signatures_len(NULL) == 0 && smh_signatures_spans(NULL) == 0 && smh_signatures_tokens(NULL) == 0);
  CHECK(smh_signatures_values_dev(NULL) == NULL);
  smh_signatures_free(NULL);
  SmhSigEntry e;
  CHECK(smh_signatures_entry(NULL, 0, &e) != 0);
  CHECK(smh_signatures_span(NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL) != 0);
  sourmash_err_clear();

  const int have = smh_device_available();
  const uint64_t len = strlen(DOC);
  SmhSignatures *sigs = smh_signatures_parse(DOC, len, NULL, 0);
  CHECK((sigs != NULL) == (have != 0));
  if (have) {
    CHECK(smh_signatures_len(sigs) == 2 && smh_signatures_tokens(sigs) == 8 && smh_signatures_spans(sigs) == 5);
    CHECK(smh_signatures_values_dev(sigs) != NULL);
    CHECK(smh_signatures_entry(sigs, 0, &e) == 0);
    CHECK(e.document == 0 && e.signature == 0 && e.sketch == 0 && e.num == 0 && e.ksize == 21 && e.seed == 42 && e.max_hash == 1000);
    CHECK(e.molecule == SMH_MOLECULE_DNA && !e.name_is_null && e.filename_is_null && e.has_abundances && e.n_mins == 3 && e.n_abundances == 3);
    CHECK(strcmp(e.name, "a [1,2] name") == 0 && strcmp(e.filename, "") == 0 && strcmp(e.license, "CC0") == 0 && strcmp(e.md5sum, "abc") == 0);
    CHECK(strcmp(e.sig_class, "sourmash_signature") == 0 && e.mins_span == 2 && e.abundances_span == 3);
    CHECK(smh_signatures_entry(sigs, 1, &e) == 0);
    CHECK(e.sketch == 1 && e.num == 500 && e.ksize == 31 && e.molecule == SMH_MOLECULE_PROTEIN && !e.has_abundances && e.n_mins == 2);
    CHECK(smh_signatures_entry(sigs, 2, &e) == 3);
    sourmash_err_clear();
    uint64_t start = 0, end = 0, first = 0, count = 0, bad = 0;
    uint32_t status = 9;
    CHECK(smh_signatures_span(sigs, 2, &start, &end, &first, &count, &status, &bad) == 0);
    CHECK(end - start == strlen("3, 5,\n9") && first == 0 && count == 3 && status == SMH_SIGSPAN_CLOSED && bad == UINT64_MAX);
    CHECK(memcmp(DOC + start, "3, 5,\n9", end - start) == 0);
    CHECK(smh_signatures_span(sigs, 5, NULL, NULL, NULL, NULL, NULL, NULL) == 3);
    sourmash_err_clear();

    /* every entry: the second node's lack of abundances decides for the index */
    SmhIndex *all = smh_signatures_index(sigs, NULL, 0);
    CHECK(all != NULL && smh_index_len(all) == 2 && !smh_index_has_abundances(all));
    uint64_t off[4] = {77, 77, 77, 77}, hashes[6] = {77, 77, 77, 77, 77, 77};
    uint32_t ab[6] = {77, 77, 77, 77, 77, 77};
    CHECK(smh_index_read(all, off, hashes, NULL) == 0 && off[0] == 0 && off[1] == 3 && off[2] == 5);
    CHECK(hashes[0] == 3 && hashes[1] == 5 && hashes[2] == 9 && hashes[3] == 7 && hashes[4] == 8 && hashes[5] == 77);
    smh_index_free(all);
    /* chosen entries, repeated */
    const uint32_t ids[2] = {0, 0};
    SmhIndex *twice = smh_signatures_index(sigs, ids, 2);
    CHECK(twice != NULL && smh_index_len(twice) == 2 && smh_index_has_abundances(twice));
    CHECK(smh_index_read(twice, off, hashes, ab) == 3 && ab[0] == 77);   /* as every index that holds such an abundance refuses */
    sourmash_err_clear();
    CHECK(smh_index_read(twice, off, hashes, NULL) == 0 && off[2] == 6 && hashes[3] == 3 && hashes[5] == 9);
    smh_index_free(twice);
    uint32_t kept[2] = {77, 77};
    CHECK(smh_signatures_filter(sigs, 0, NULL, NULL) == 2 && smh_signatures_filter(sigs, 31, "Protein", kept) == 1 && kept[0] == 1 && kept[1] == 77);
    CHECK(smh_signatures_filter(sigs, 0, "rna", kept) == 0 && smh_signatures_filter(sigs, 21, "dna", kept) == 1 && kept[0] == 0);
    SmhIndex *prot = smh_signatures_index_filtered(sigs, 31, "Protein");
    CHECK(prot != NULL && smh_index_len(prot) == 1);
    smh_index_free(prot);
    SmhIndex *none = smh_signatures_index_filtered(sigs, 51, NULL);
    CHECK(none != NULL && smh_index_len(none) == 0);
    smh_index_free(none);
    const uint32_t beyond[1] = {2};
    CHECK(smh_signatures_index(sigs, beyond, 1) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    CHECK(smh_signatures_index(NULL, NULL, 0) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    smh_signatures_free(sigs);

    /* refusals: a document the host loader refuses, a float split in two, hashes that do not ascend */
    const char *cut = "[{\"signatures\":[1,]}]";
    CHECK(smh_signatures_parse(cut, strlen(cut), NULL, 0) == NULL && sourmash_err_get_last_code() == 100004);
    sourmash_err_clear();
    const char *flt = "[{\"x\":[1.5]}]";
    CHECK(smh_signatures_parse(flt, strlen(flt), NULL, 0) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    const uint64_t short_offsets[2] = {1, (uint64_t)strlen(cut)};      /* the documents must tile the text */
    CHECK(smh_signatures_parse(cut, strlen(cut), short_offsets, 1) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    const uint64_t bad_offsets[2] = {0, 1000};
    CHECK(smh_signatures_parse(cut, strlen(cut), bad_offsets, 1) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    CHECK(smh_signatures_parse_dev(NULL, 5, NULL, 0, NULL) == NULL);
    sourmash_err_clear();
    const char *unsorted =
        "[{\"hash_function\":\"0.murmur64\",\"signatures\":[{\"num\":0,\"ksize\":21,\"seed\":42,\"max_hash\":9,\"mins\":[3,3],\"md5sum\":\"\","
        "\"molecule\":\"DNA\"}]}]";
    sigs = smh_signatures_parse(unsorted, strlen(unsorted), NULL, 0);
    CHECK(sigs != NULL && smh_signatures_len(sigs) == 1);
    CHECK(smh_signatures_index(sigs, NULL, 0) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    smh_signatures_free(sigs);
  } else {
    CHECK(sourmash_err_get_last_code() == 2);
    sourmash_err_clear();
    CHECK(smh_signatures_parse_dev(NULL, 0, NULL, 0, NULL) == NULL && sourmash_err_get_last_code() == 2);
    sourmash_err_clear();
    CHECK(smh_signatures_index(NULL, NULL, 0) == NULL && sourmash_err_get_last_code() == 2);
    sourmash_err_clear();
    CHECK(smh_signatures_index_filtered(NULL, 0, NULL) == NULL && sourmash_err_get_last_code() == 2);
    sourmash_err_clear();
    CHECK(smh_signatures_filter(NULL, 0, NULL, NULL) == 0);
  }
  sourmash_err_clear();
  printf("sigscan abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
