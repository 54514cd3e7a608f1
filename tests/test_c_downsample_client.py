"""The downsampling symbols that the Rust shim binds, link-checked from C like the rest of the shim (tests/test_c_client.py):
tests/c_downsample_symbols.c compiles with -Werror against the headers, links, calls each one.  Its host cuts run
everywhere; its index and block calls run where there is a device."""
import os
import re

import pytest

import test_c_client as base

BOUND = {"smh_kmerminhash_downsample_max_hash", "smh_kmerminhash_downsample_num", "smh_index_downsample",
         "smh_index_max_hash_range", "smh_downsample_block_dev", "smh_downsample_geometry"}


def test_downsample_forwards_are_link_checked(pkg, tmp_path):
    shim = open(os.path.join(base.ROOT, "sourmash-rust_amd", "rust", "src", "lib.rs")).read()
    block = shim[shim.index("link-checked by tests/c_downsample_symbols.c"):]
    block = block[:block.index("\n}\n")]
    bound = set(re.findall(r"\bfn (smh_[a-z0-9_]+)\(", block))
    assert bound == BOUND
    ctext = open(os.path.join(base.ROOT, "tests", "c_downsample_symbols.c")).read()
    assert not [sym for sym in bound if not re.search(r"\b%s\(" % sym, ctext)]
    assert bound <= set(pkg.exported_symbols())
    assert "downsample abi client ok" in base._build_and_run(pkg, tmp_path, "c_downsample_symbols")
    for sig in ("pub fn downsample_max_hash(&self, max_hash: u64) -> Result<KmerMinHash, Error>",
                "pub fn downsample_num(&self, num: u32) -> Result<KmerMinHash, Error>"):
        assert sig in shim, sig


@pytest.mark.gpu
def test_downsample_link_check_on_the_gpu(pkg, tmp_path):
    assert "downsample abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_downsample_symbols")
