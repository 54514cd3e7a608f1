"""The entry points of building an index from records and of concatenation, link-checked from C like the rest of the additive
ABI (tests/test_c_client.py): tests/c_index_build_symbols.c compiles with -Werror against the headers, links, calls each one.
Without a GPU every refusal of the arguments still returns MSG -- it precedes the device -- and a valid call returns 2."""
import os
import re

import pytest

import test_c_client as base

SYMBOLS = {"smh_index_from_sequences", "smh_index_from_sequences_dev", "smh_index_from_records", "smh_index_concat",
           "smh_index_build_set_budget", "smh_index_build_budget", "smh_index_build_geometry"}


def test_index_build_symbols_are_declared_exported_and_link_checked(pkg, tmp_path):
    header = open(os.path.join(base.ROOT, "include", "sourmash_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(smh_index_from_[a-z0-9_]*|smh_index_concat|smh_index_build_[a-z0-9_]*)\(", code))
    assert declared == SYMBOLS
    assert "SMH_INPUT_NUCLEOTIDE = 0" in header and "SMH_INPUT_AMINO = 1" in header
    ctext = open(os.path.join(base.ROOT, "tests", "c_index_build_symbols.c")).read()
    assert not [sym for sym in SYMBOLS if not re.search(r"\b%s\(" % sym, ctext)]
    assert SYMBOLS <= set(pkg.exported_symbols())
    assert "index build abi client ok" in base._build_and_run(pkg, tmp_path, "c_index_build_symbols")


@pytest.mark.gpu
def test_index_build_three_records_through_plain_c(pkg, tmp_path):
    assert "index build abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_index_build_symbols")
