/* Link check of the downsampling entry points the Rust shim binds (sourmash-rust_amd/rust/src/lib.rs, fourth extern
 * block): each is called with the header's prototype, the way the shim calls it.  Needs no GPU: the cuts of host-resident
 * sketches are made on the host; with a device the index and block calls succeed, without one they report 2. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(void) {
  const uint64_t mx = 1ull << 60;
  KmerMinHash *sc = kmerminhash_new(0, 21, false, 42, mx, true);
  KmerMinHash *nm = kmerminhash_new(4, 21, false, 42, 0, false);
  CHECK(sc && nm);
  const uint64_t h[4] = {5, 9, 100, 1ull << 59};
  for (int i = 0; i < 4; i++) {
    kmerminhash_mins_push(sc, h[i]);
    kmerminhash_abunds_push(sc, (uint64_t)i + 1);
    kmerminhash_mins_push(nm, h[i]);
  }
  KmerMinHash *cut = smh_kmerminhash_downsample_max_hash(sc, 100);
  CHECK(cut && kmerminhash_max_hash(cut) == 100 && kmerminhash_num(cut) == 0 && kmerminhash_ksize(cut) == 21);
  CHECK(kmerminhash_get_mins_size(cut) == 3 && kmerminhash_get_min_idx(cut, 2) == 100 && kmerminhash_get_abund_idx(cut, 2) == 3);
  kmerminhash_free(cut);
  cut = smh_kmerminhash_downsample_max_hash(sc, 99);
  CHECK(cut && kmerminhash_get_mins_size(cut) == 2);
  kmerminhash_free(cut);
  CHECK(smh_kmerminhash_downsample_max_hash(sc, 0) == NULL && sourmash_err_get_last_code() == SOURMASH_ERROR_CODE_MSG);
  sourmash_err_clear();
  CHECK(smh_kmerminhash_downsample_max_hash(sc, mx + 1) == NULL && sourmash_err_get_last_code() == SOURMASH_ERROR_CODE_MSG);
  sourmash_err_clear();
  CHECK(smh_kmerminhash_downsample_max_hash(nm, 5) == NULL && sourmash_err_get_last_code() == SOURMASH_ERROR_CODE_MSG);
  sourmash_err_clear();
  cut = smh_kmerminhash_downsample_num(nm, 2);
  CHECK(cut && kmerminhash_num(cut) == 2 && kmerminhash_get_mins_size(cut) == 2 && kmerminhash_get_min_idx(cut, 1) == 9);
  kmerminhash_free(cut);
  CHECK(smh_kmerminhash_downsample_num(nm, 5) == NULL && sourmash_err_get_last_code() == SOURMASH_ERROR_CODE_MSG);
  sourmash_err_clear();
  CHECK(smh_kmerminhash_downsample_num(sc, 1) == NULL && sourmash_err_get_last_code() == SOURMASH_ERROR_CODE_MSG);
  sourmash_err_clear();

  uint32_t tile = 0, threads = 0;
  smh_downsample_geometry(&tile, &threads);
  CHECK(tile > 0 && threads > 0 && threads % 64 == 0 && tile % threads == 0);

  const int have = smh_device_available();
  KmerMinHash *nodes[2] = {sc, sc};
  SmhIndex *idx = smh_index_new(nodes, 2);
  CHECK((idx != NULL) == (have != 0));
  sourmash_err_clear();
  const uint64_t off[1] = {0};
  uint64_t new_off[1] = {7};
  const int rc = smh_downsample_block_dev(NULL, NULL, off, 0, 100, NULL, NULL, 0, new_off, NULL);
  CHECK(rc == (have ? 0 : 2));
  sourmash_err_clear();
  if (have) {
    CHECK(new_off[0] == 0);
    uint64_t lo = 0, hi = 0;
    CHECK(smh_index_max_hash_range(idx, &lo, &hi) == 0 && lo == mx && hi == mx);
    SmhIndex *child = smh_index_downsample(idx, 100);
    CHECK(child && smh_index_len(child) == 2);
    CHECK(smh_index_max_hash_range(child, &lo, &hi) == 0 && lo == 100 && hi == 100);
    CHECK(smh_index_has_abundances(child));
    uint64_t norms[2] = {0, 0};
    CHECK(smh_index_norms2(child, norms) == 0 && norms[0] == 14 && norms[1] == 14);
    CHECK(smh_index_downsample(idx, mx + 1) == NULL && sourmash_err_get_last_code() == SOURMASH_ERROR_CODE_MSG);
    sourmash_err_clear();
    smh_index_free(child);
    smh_index_free(idx);
  }
  kmerminhash_free(sc);
  kmerminhash_free(nm);
  printf("downsample abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
