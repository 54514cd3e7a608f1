"""The entry points of filtering an index and of taking a subset of its nodes, link-checked from C like the rest of the
additive ABI (tests/test_c_client.py): tests/c_filter_symbols.c compiles with -Werror against the headers, links, calls each
one."""
import os
import re

import pytest

import test_c_client as base

SYMBOLS = {"smh_index_filter", "smh_index_select", "smh_filter_geometry"}


def test_filter_symbols_are_declared_exported_and_link_checked(pkg, tmp_path):
    header = open(os.path.join(base.ROOT, "include", "sourmash_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(smh_index_filter|smh_index_select|smh_filter_[a-z0-9_]*)\(", code))
    assert declared == SYMBOLS
    assert "SMH_FILTER_OPERAND_NONE = 0, SMH_FILTER_KEEP_IN = 1, SMH_FILTER_DROP_IN = 2" in header
    assert "SMH_FILTER_ABUND_OWN = 0, SMH_FILTER_ABUND_FLAT = 1, SMH_FILTER_ABUND_OPERAND = 2" in header
    ctext = open(os.path.join(base.ROOT, "tests", "c_filter_symbols.c")).read()
    assert not [sym for sym in SYMBOLS if not re.search(r"\b%s\(" % sym, ctext)]
    assert SYMBOLS <= set(pkg.exported_symbols())
    assert "filter abi client ok" in base._build_and_run(pkg, tmp_path, "c_filter_symbols")


@pytest.mark.gpu
def test_filter_four_node_answer_through_plain_c(pkg, tmp_path):
    assert "filter abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_filter_symbols")
