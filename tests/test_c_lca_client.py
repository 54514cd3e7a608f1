"""The taxonomic LCA entry points, link-checked from C like the rest of the additive ABI (tests/test_c_client.py):
tests/c_lca_symbols.c compiles with -Werror against the headers, links, calls each one."""
import os
import re

import pytest

import test_c_client as base

SYMBOLS = {"smh_lca_check_taxonomy", "smh_index_set_taxonomy", "smh_index_has_taxonomy", "smh_index_lca_many", "smh_index_lca_block_dev",
           "smh_index_lca_sequences", "smh_index_lca_sequences_dev", "smh_index_lca_records", "smh_lca_geometry", "smh_lca_set_budget",
           "smh_lca_budget"}


def test_lca_symbols_are_declared_exported_and_link_checked(pkg, tmp_path):
    header = open(os.path.join(base.ROOT, "include", "sourmash_amd.h")).read()
    declared = set(re.findall(r"\b(smh_[a-z0-9_]*(?:lca|taxonomy)[a-z0-9_]*)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == SYMBOLS
    assert not [s for s in SYMBOLS if s.startswith(("smh_match_", "smh_index_match_", "smh_gather_", "smh_index_gather_"))]
    assert "typedef struct SmhLcaRow" in header and "#define SMH_NO_TAXON 0xffffffffu" in header
    ctext = open(os.path.join(base.ROOT, "tests", "c_lca_symbols.c")).read()
    assert not [sym for sym in SYMBOLS if not re.search(r"\b%s\(" % sym, ctext)]
    assert SYMBOLS <= set(pkg.exported_symbols())
    assert "lca abi client ok" in base._build_and_run(pkg, tmp_path, "c_lca_symbols")


@pytest.mark.gpu
def test_lca_three_node_answer_through_plain_c(pkg, tmp_path):
    assert "lca abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_lca_symbols")
