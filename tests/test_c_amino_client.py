"""The alphabet / amino-acid symbols that the Rust shim binds, link-checked from C like the rest of the shim
(tests/test_c_client.py): tests/c_amino_symbols.c compiles with -Werror against the headers, links, calls each one."""
import os
import re

import test_c_client as base


def test_amino_forwards_are_link_checked(pkg, tmp_path):
    shim = open(os.path.join(base.ROOT, "sourmash-rust_amd", "rust", "src", "lib.rs")).read()
    block = shim[shim.index("link-checked by tests/c_amino_symbols.c"):]
    block = block[:block.index("\n}\n")]
    bound = set(re.findall(r"\bfn (smh_[a-z0-9_]+)\(", block))
    assert bound == {"smh_kmerminhash_new_molecule", "smh_kmerminhash_molecule", "smh_add_protein", "smh_add_proteins",
                     "smh_add_proteins_dev", "smh_add_records_protein", "smh_amino_geometry"}
    ctext = open(os.path.join(base.ROOT, "tests", "c_amino_symbols.c")).read()
    assert not [sym for sym in bound if not re.search(r"\b%s\(" % sym, ctext)]
    assert bound <= set(pkg.exported_symbols())
    assert "amino abi client ok" in base._build_and_run(pkg, tmp_path, "c_amino_symbols")
    for sig in ("pub fn new_molecule(num: u32, ksize: u32, molecule: Molecule, seed: u64, max_hash: u64, track_abundance: bool) -> KmerMinHash",
                "pub fn add_protein(&mut self, seq: &[u8]) -> Result<(), Error>",
                "pub fn add_proteins(&mut self, seq: &[u8], offsets: &[u64]) -> Result<(), Error>"):
        assert sig in shim, sig
