"""The entry points of signature JSON read on the device, link-checked from C like the rest of the additive ABI
(tests/test_c_client.py): tests/c_sigscan_symbols.c compiles with -Werror against the headers, links, calls each one."""
import os
import re

import pytest

import test_c_client as base

SYMBOLS = {"smh_signatures_parse", "smh_signatures_parse_dev", "smh_signatures_free", "smh_signatures_len", "smh_signatures_spans",
           "smh_signatures_tokens", "smh_signatures_entry", "smh_signatures_span", "smh_signatures_values_dev", "smh_signatures_index", "smh_signatures_filter",
           "smh_signatures_index_filtered", "smh_sigscan_geometry"}


def test_sigscan_symbols_are_declared_exported_and_link_checked(pkg, tmp_path):
    header = open(os.path.join(base.ROOT, "include", "sourmash_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(smh_signatures_[a-z0-9_]*|smh_sigscan_[a-z0-9_]*)\(", code))
    assert declared == SYMBOLS
    assert "SMH_SIGSPAN_CLOSED = 0, SMH_SIGSPAN_OPEN = 1, SMH_SIGSPAN_OVERFLOW = 2, SMH_SIGSPAN_BAD_SYNTAX = 3" in header
    ctext = open(os.path.join(base.ROOT, "tests", "c_sigscan_symbols.c")).read()
    assert not [sym for sym in SYMBOLS if not re.search(r"\b%s\(" % sym, ctext)]
    assert SYMBOLS <= set(pkg.exported_symbols())
    assert "sigscan abi client ok" in base._build_and_run(pkg, tmp_path, "c_sigscan_symbols")


@pytest.mark.gpu
def test_sigscan_two_sketch_answer_through_plain_c(pkg, tmp_path):
    assert "sigscan abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_sigscan_symbols")
