/* Link check of the alphabet / amino-acid entry points the Rust shim binds (sourmash-rust_amd/rust/src/lib.rs, second
 * extern block): each is called with the header's prototype, the way the shim calls it.  Needs no GPU: with one the
 * sketching calls succeed, without one they return 2 and leave the sketch alone. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(void) {
  const char *rec = "MVLSPADKTNVKAAWGKVGAHAGEYGAEALERMFLSFPTTKTYFPHF*xb";
  const uint64_t len = strlen(rec), off[2] = {0, len};
  KmerMinHash *dna = smh_kmerminhash_new_molecule(1000, 27, SMH_MOLECULE_DNA, 42, 0, true);
  KmerMinHash *dh = smh_kmerminhash_new_molecule(1000, 27, SMH_MOLECULE_DAYHOFF, 42, 0, true);
  CHECK(dna && dh);
  CHECK(smh_kmerminhash_molecule(dna) == SMH_MOLECULE_DNA && smh_kmerminhash_molecule(dh) == SMH_MOLECULE_DAYHOFF);
  CHECK(!kmerminhash_is_protein(dna) && kmerminhash_is_protein(dh));
  CHECK(smh_add_protein(dna, rec, len) == 3);
  CHECK(smh_add_proteins(dna, rec, off, 1) == 3);
  CHECK(smh_add_proteins_dev(dna, NULL, 0, off, 0, NULL) == 3);
  CHECK(smh_add_records_protein(dna, NULL) == 3);
  sourmash_err_clear();
  const int have = smh_device_available();
  const int rc = smh_add_protein(dh, rec, len);
  CHECK(rc == (have ? 0 : 2));
  CHECK(smh_add_proteins(dh, rec, off, 1) == rc);
  CHECK(kmerminhash_get_mins_size(dh) == (have ? 42u : 0u));
  if (have) CHECK(kmerminhash_get_min_idx(dh, 0) == 1192610630844060659ull);
  sourmash_err_clear();
  uint32_t tile = 0, run = 0;
  smh_amino_geometry(len, 9, &tile, &run);
  CHECK(tile > 0 && run > 0 && tile % run == 0);
  kmerminhash_free(dna);
  kmerminhash_free(dh);
  printf("amino abi client ok\n");
  return 0;
}
