/* Link check of zip collections (include/sourmash_amd.h, "Zip collections"): each entry point is called with the header's
 * prototype.  The scan needs no GPU: an archive of two stored entries spelled out here (a.sig, and e.sig with the encrypted
 * flag) is scanned from plain C, every field is compared, and the scan's refusals are met.  The device calls are taken as far
 * as plain C can take them without device memory of its own: with a GPU an empty list of ids succeeds and every refusal that
 * comes before a launch is met; without one they fail with 2 in the error slot. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static const uint8_t ZIP[198] = {
    0x50,0x4b,0x03,0x04,0x14,0x00,0x00,0x00,0x00,0x00,0x00,0x00,0x21,0x00,0x29,0xbb,0x4c,0x0d,0x02,0x00,0x00,0x00,0x02,0x00,0x00,0x00,0x05,0x00,
    0x00,0x00,0x61,0x2e,0x73,0x69,0x67,0x5b,0x5d,0x50,0x4b,0x03,0x04,0x14,0x00,0x01,0x00,0x00,0x00,0x00,0x00,0x21,0x00,0x29,0xbb,0x4c,0x0d,0x02,
    0x00,0x00,0x00,0x02,0x00,0x00,0x00,0x05,0x00,0x00,0x00,0x65,0x2e,0x73,0x69,0x67,0x5b,0x5d,0x50,0x4b,0x01,0x02,0x14,0x00,0x14,0x00,0x00,0x00,
    0x00,0x00,0x00,0x00,0x21,0x00,0x29,0xbb,0x4c,0x0d,0x02,0x00,0x00,0x00,0x02,0x00,0x00,0x00,0x05,0x00,0x00,0x00,0x00,0x00,0x00,0x00,0x00,0x00,
    0x00,0x00,0x00,0x00,0x00,0x00,0x00,0x00,0x61,0x2e,0x73,0x69,0x67,0x50,0x4b,0x01,0x02,0x14,0x00,0x14,0x00,0x01,0x00,0x00,0x00,0x00,0x00,0x21,
    0x00,0x29,0xbb,0x4c,0x0d,0x02,0x00,0x00,0x00,0x02,0x00,0x00,0x00,0x05,0x00,0x00,0x00,0x00,0x00,0x00,0x00,0x00,0x00,0x00,0x00,0x00,0x00,0x25,
    0x00,0x00,0x00,0x65,0x2e,0x73,0x69,0x67,0x50,0x4b,0x05,0x06,0x00,0x00,0x00,0x00,0x02,0x00,0x02,0x00,0x66,0x00,0x00,0x00,0x4a,0x00,0x00,0x00,
    0x00,0x00};

int main(void) {
  uint32_t chunk = 0, threads = 0;
  smh_archive_geometry(&chunk, &threads);
  CHECK(chunk >= 64 && threads >= 64 && threads % 64 == 0);
  smh_archive_geometry(NULL, NULL);
  CHECK(smh_archive_sorted() == 1);
  smh_archive_set_sorted(0);
  CHECK(smh_archive_sorted() == 0);
  smh_archive_set_sorted(1);
  /* a NULL handle */
  CHECK(smh_archive_entries(NULL) == 0);
  smh_archive_free(NULL);
  SmhArchiveEntry e;
  CHECK(smh_archive_entry(NULL, 0, &e) != 0);
  sourmash_err_clear();

  SmhArchive *a = smh_archive_scan(ZIP, sizeof ZIP);
  CHECK(a != NULL && smh_archive_entries(a) == 2);
  CHECK(smh_archive_entry(a, 0, &e) == 0);
  CHECK(strcmp(e.name, "a.sig") == 0 && e.reason[0] == 0 && e.method == 0 && e.flags == 0 && e.crc32 == 0x0d4cbb29u);
  CHECK(e.kind == SMH_ARCHIVE_STORED && e.device_ok == 1 && e.comp_size == 2 && e.size == 2 && e.header_off == 0 && e.data_off == 35);
  CHECK(e.payload_off == 35 && e.payload_len == 2 && e.text_size == 2 && e.text_crc == 0x0d4cbb29u);
  CHECK(memcmp(ZIP + e.data_off, "[]", 2) == 0);
  CHECK(smh_archive_entry(a, 1, &e) == 0);
  CHECK(strcmp(e.name, "e.sig") == 0 && e.flags == 1 && e.device_ok == 0 && strcmp(e.reason, "encrypted entry") == 0 && e.data_off == 72);
  CHECK(smh_archive_entry(a, 2, &e) == 3);
  sourmash_err_clear();
  /* the scan's refusals: code 3, "archive: ..." */
  CHECK(smh_archive_scan(ZIP, sizeof ZIP - 1) == NULL && sourmash_err_get_last_code() == 3);
  SourmashStr msg = sourmash_err_get_last_message();
  CHECK(msg.len > 9 && memcmp(msg.data, "archive: ", 9) == 0);
  sourmash_str_free(&msg);
  sourmash_err_clear();
  CHECK(smh_archive_scan(NULL, 0) == NULL && sourmash_err_get_last_code() == 3);
  sourmash_err_clear();

  const int have = smh_device_available();
  const uint32_t ids[2] = {0, 1}, far[1] = {7};
  const uint64_t offs[2] = {0, 2};
  uint8_t status[2] = {9, 9};
  if (have) {
    CHECK(smh_archive_inflate(a, ZIP, sizeof ZIP, NULL, NULL, 0, NULL, 0, 1, NULL) == 0);
    CHECK(smh_archive_inflate_dev(a, NULL, sizeof ZIP, NULL, NULL, 0, NULL, 0, 1, NULL, NULL) == 0);
    /* refused before anything is launched: another length, an id past the entries, an entry that is not for the device, a
     * slice that leaves the output */
    CHECK(smh_archive_inflate_dev(a, NULL, sizeof ZIP - 1, ids, offs, 1, NULL, 2, 1, status, NULL) == 3);
    sourmash_err_clear();
    CHECK(smh_archive_inflate(a, ZIP, sizeof ZIP, far, offs, 1, NULL, 2, 1, status) == 3);
    sourmash_err_clear();
    CHECK(smh_archive_inflate(a, ZIP, sizeof ZIP, ids, offs, 2, NULL, 4, 1, status) == 3);
    msg = sourmash_err_get_last_message();
    CHECK(msg.len > 0 && memmem(msg.data, msg.len, "encrypted entry", 15) != NULL && memmem(msg.data, msg.len, "(entry 1 'e.sig')", 17) != NULL);
    sourmash_str_free(&msg);
    sourmash_err_clear();
    CHECK(smh_archive_inflate(a, ZIP, sizeof ZIP, ids, offs, 1, NULL, 1, 1, status) == 3);
    sourmash_err_clear();
    CHECK(status[0] == 9 && status[1] == 9);
  } else {
    CHECK(smh_archive_inflate(a, ZIP, sizeof ZIP, ids, offs, 1, NULL, 2, 1, status) == 2);
    sourmash_err_clear();
    CHECK(smh_archive_inflate_dev(a, NULL, sizeof ZIP, ids, offs, 1, NULL, 2, 1, status, NULL) == 2);
  }
  sourmash_err_clear();
  smh_archive_free(a);
  printf("archive abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
