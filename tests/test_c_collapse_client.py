"""The entry points of collapsing an index by groups and of the read-back, link-checked from C like the rest of the additive
ABI (tests/test_c_client.py): tests/c_collapse_symbols.c compiles with -Werror against the headers, links, calls each one."""
import os
import re

import pytest

import test_c_client as base

SYMBOLS = {"smh_index_collapse", "smh_collapse_geometry", "smh_index_read"}


def test_collapse_symbols_are_declared_exported_and_link_checked(pkg, tmp_path):
    header = open(os.path.join(base.ROOT, "include", "sourmash_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(smh_[a-z0-9_]*collapse[a-z0-9_]*|smh_index_read)\(", code))
    assert declared == SYMBOLS
    assert "SMH_COLLAPSE_FLAT = 0" in header and "SMH_COLLAPSE_SUM = 1" in header and "SMH_COLLAPSE_COUNT = 2" in header
    assert "#define SMH_COLLAPSE_DROP 0xffffffffu" in header
    ctext = open(os.path.join(base.ROOT, "tests", "c_collapse_symbols.c")).read()
    assert not [sym for sym in SYMBOLS if not re.search(r"\b%s\(" % sym, ctext)]
    assert SYMBOLS <= set(pkg.exported_symbols())
    assert "collapse abi client ok" in base._build_and_run(pkg, tmp_path, "c_collapse_symbols")


@pytest.mark.gpu
def test_collapse_four_node_answer_through_plain_c(pkg, tmp_path):
    assert "collapse abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_collapse_symbols")
