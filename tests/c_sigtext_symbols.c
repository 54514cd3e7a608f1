/* Link check of signature JSON written on the device (include/sourmash_amd.h, "Signature JSON written on the device"): each
 * entry point is called with the header's prototype.  Needs no GPU: with one an index of two sketches is written from plain C,
 * compared byte for byte with the text spelled out here, and every refusal is met; without one the device calls fail with 2 in
 * the error slot and the accessors answer for a NULL handle. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

/* the md5sums: md5("21359") and md5("21"), computed with Python's hashlib */
static const char *WANT =
    "[{\"class\":\"sourmash_signature\",\"email\":\"\",\"hash_function\":\"0.murmur64\",\"filename\":null,\"name\":\"a \\\"b\\\" \\\\ \\u0001\","
    "\"license\":\"CC0\",\"signatures\":[{\"num\":0,\"ksize\":21,\"seed\":42,\"max_hash\":1000,\"mins\":[3,5,9],"
    "\"md5sum\":\"0c5bcd68aebc9060a7f2e5047bb962de\",\"abundances\":[1,20,4294967295],\"molecule\":\"DNA\"}],\"version\":0.4}]"
    "[]"
    "[{\"class\":\"sourmash_signature\",\"email\":\"\",\"hash_function\":\"0.murmur64\",\"filename\":\"f.fa\",\"name\":null,"
    "\"license\":\"CC0\",\"signatures\":[{\"num\":0,\"ksize\":21,\"seed\":42,\"max_hash\":1000,\"mins\":[],"
    "\"md5sum\":\"3c59dc048e8850243be8079a5c74d079\",\"abundances\":[],\"molecule\":\"DNA\"}],\"version\":0.4}]";

static int hex_equal(const uint8_t *digest, const char *hex) {
  char got[33];
  for (int i = 0; i < 16; i++) sprintf(got + 2 * i, "%02x", digest[i]);
  return memcmp(got, hex, 32) == 0;
}

int main(void) {
  uint32_t tile = 0, threads = 0, step = 0;
  smh_sigtext_geometry(&tile, &threads, &step);
  CHECK(tile >= 64 && threads >= 64 && threads % 64 == 0 && tile % threads == 0 && step >= 1);
  smh_sigtext_geometry(NULL, NULL, NULL);
  /* a NULL handle */
  CHECK(smh_sigtext_len(NULL) == 0 && smh_sigtext_documents(NULL) == 0 && smh_sigtext_dev(NULL) == NULL);
  smh_sigtext_free(NULL);
  uint64_t offs[8];
  char buf[2048];
  CHECK(smh_sigtext_doc_offsets(NULL, offs) != 0);
  sourmash_err_clear();
  CHECK(smh_sigtext_read(NULL, 0, 0, buf) != 0);
  sourmash_err_clear();

  const int have = smh_device_available();
  uint8_t digests[32];
  if (have) {
    KmerMinHash *a = kmerminhash_new(0, 21, false, 42, 1000, true), *b = kmerminhash_new(0, 21, false, 42, 1000, true);
    const uint64_t h[3] = {3, 5, 9}, ab[3] = {1, 20, 4294967295ull};
    for (int i = 0; i < 3; i++) { kmerminhash_mins_push(a, h[i]); kmerminhash_abunds_push(a, ab[i]); }
    KmerMinHash *nodes[2] = {a, b};
    SmhIndex *idx = smh_index_new(nodes, 2);
    CHECK(idx != NULL && smh_index_len(idx) == 2 && smh_index_has_abundances(idx));
    CHECK(smh_index_md5(idx, digests) == 0);
    CHECK(hex_equal(digests + 16, "3c59dc048e8850243be8079a5c74d079"));   /* md5("21") */
    const char *names[2] = {"a \"b\" \\ \x01", NULL}, *filenames[2] = {NULL, "f.fa"};
    const uint32_t docs[4] = {0, 1, 1, 2};
    SmhSigText *t = smh_index_sigtext(idx, names, filenames, docs, 3);
    CHECK(t != NULL && smh_sigtext_documents(t) == 3 && smh_sigtext_dev(t) != NULL);
    const uint64_t len = smh_sigtext_len(t);
    CHECK(len == strlen(WANT) && len < sizeof buf);
    CHECK(smh_sigtext_read(t, 0, len, buf) == 0);
    CHECK(memcmp(buf, WANT, len) == 0);
    CHECK(hex_equal(digests, "0c5bcd68aebc9060a7f2e5047bb962de"));
    CHECK(smh_sigtext_doc_offsets(t, offs) == 0 && offs[0] == 0 && offs[2] == offs[1] + 2 && offs[3] == len);
    CHECK(buf[offs[1]] == '[' && buf[offs[1] + 1] == ']' && buf[offs[2]] == '[');
    char two[2];
    CHECK(smh_sigtext_read(t, offs[1], 2, two) == 0 && two[0] == '[' && two[1] == ']');
    CHECK(smh_sigtext_read(t, len, 1, two) == 3);
    sourmash_err_clear();
    smh_sigtext_free(t);
    /* one document, no names */
    t = smh_index_sigtext(idx, NULL, NULL, NULL, 0);
    CHECK(t != NULL && smh_sigtext_documents(t) == 1);
    smh_sigtext_free(t);
    /* refusals: doc_starts */
    const uint32_t late[2] = {1, 2}, shrt[2] = {0, 1}, down[4] = {0, 2, 1, 2};
    CHECK(smh_index_sigtext(idx, NULL, NULL, late, 1) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    CHECK(smh_index_sigtext(idx, NULL, NULL, shrt, 1) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    CHECK(smh_index_sigtext(idx, NULL, NULL, down, 3) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    CHECK(smh_index_sigtext(NULL, NULL, NULL, NULL, 0) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    CHECK(smh_index_md5(NULL, digests) == 3);
    sourmash_err_clear();
    smh_index_free(idx);
    /* an abundance of 2^32: the text is refused, the md5 is not */
    kmerminhash_mins_push(b, 7); kmerminhash_abunds_push(b, 4294967296ull);
    idx = smh_index_new(nodes, 2);
    CHECK(idx != NULL);
    CHECK(smh_index_sigtext(idx, NULL, NULL, NULL, 0) == NULL && sourmash_err_get_last_code() == 3);
    sourmash_err_clear();
    CHECK(smh_index_md5(idx, digests) == 0);
    smh_index_free(idx);
    kmerminhash_free(a); kmerminhash_free(b);
  } else {
    CHECK(smh_index_sigtext(NULL, NULL, NULL, NULL, 0) == NULL && sourmash_err_get_last_code() == 2);
    sourmash_err_clear();
    CHECK(smh_index_md5(NULL, digests) == 2);
  }
  sourmash_err_clear();
  printf("sigtext abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
