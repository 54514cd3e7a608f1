"""The batch search entry points, link-checked from C like the rest of the additive ABI (tests/test_c_client.py):
tests/c_search_many_symbols.c compiles with -Werror against the headers, links, calls each one."""
import os
import re

import pytest

import test_c_client as base

SYMBOLS = {"smh_index_search_many", "smh_index_search_block_dev", "smh_index_search_self", "smh_search_many_set_budget",
           "smh_search_many_budget", "smh_search_geometry"}


def test_search_symbols_are_declared_exported_and_link_checked(pkg, tmp_path):
    header = open(os.path.join(base.ROOT, "include", "sourmash_amd.h")).read()
    declared = set(re.findall(r"\b(smh_[a-z0-9_]*search[a-z0-9_]*)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == SYMBOLS
    assert "typedef struct SmhSearchRow" in header and "SMH_SEARCH_MAX_CONTAINMENT = 3" in header
    ctext = open(os.path.join(base.ROOT, "tests", "c_search_many_symbols.c")).read()
    assert not [sym for sym in SYMBOLS if not re.search(r"\b%s\(" % sym, ctext)]
    assert SYMBOLS <= set(pkg.exported_symbols())
    assert "search_many abi client ok" in base._build_and_run(pkg, tmp_path, "c_search_many_symbols")


@pytest.mark.gpu
def test_search_three_node_answer_through_plain_c(pkg, tmp_path):
    assert "search_many abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_search_many_symbols")
