"""The entry points of zip collections, link-checked from C like the rest of the additive ABI (tests/test_c_client.py):
tests/c_archive_symbols.c compiles with -Werror against the headers, links, calls each one."""
import os
import re

import pytest

import test_c_client as base

SYMBOLS = {"smh_archive_scan", "smh_archive_free", "smh_archive_entries", "smh_archive_entry", "smh_archive_inflate_dev", "smh_archive_inflate",
           "smh_archive_geometry", "smh_archive_set_sorted", "smh_archive_sorted"}


def test_archive_symbols_are_declared_exported_and_link_checked(pkg, tmp_path):
    header = open(os.path.join(base.ROOT, "include", "sourmash_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(smh_archive_[a-z0-9_]*)\(", code))
    assert declared == SYMBOLS
    ctext = open(os.path.join(base.ROOT, "tests", "c_archive_symbols.c")).read()
    assert not [sym for sym in SYMBOLS if not re.search(r"\b%s\(" % sym, ctext)]
    assert SYMBOLS <= set(pkg.exported_symbols())
    assert "archive abi client ok" in base._build_and_run(pkg, tmp_path, "c_archive_symbols")


@pytest.mark.gpu
def test_archive_refusals_through_plain_c(pkg, tmp_path):
    assert "archive abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_archive_symbols")
