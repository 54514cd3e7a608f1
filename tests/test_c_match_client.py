"""The entry points that match records against a resident index, link-checked from C like the rest of the additive ABI
(tests/test_c_client.py): tests/c_match_symbols.c compiles with -Werror against the headers, links, calls each one."""
import os
import re

import pytest

import test_c_client as base

SYMBOLS = {"smh_index_match_sequences", "smh_index_match_sequences_dev", "smh_index_match_records", "smh_match_geometry",
           "smh_match_set_pair_budget", "smh_match_pair_budget"}


def test_match_symbols_are_declared_exported_and_link_checked(pkg, tmp_path):
    header = open(os.path.join(base.ROOT, "include", "sourmash_amd.h")).read()
    declared = set(re.findall(r"\b(smh_(?:index_)?match_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == SYMBOLS
    assert "typedef struct SmhMatchRow" in header
    ctext = open(os.path.join(base.ROOT, "tests", "c_match_symbols.c")).read()
    assert not [sym for sym in SYMBOLS if not re.search(r"\b%s\(" % sym, ctext)]
    assert SYMBOLS <= set(pkg.exported_symbols())
    assert "match abi client ok" in base._build_and_run(pkg, tmp_path, "c_match_symbols")


def test_geometry_and_budget_need_no_device(pkg):
    lds_pairs, threads, samples = pkg.matrix.match_geometry()
    assert lds_pairs > 0 and threads % 64 == 0 and samples > 0
    default = pkg.matrix.match_pair_budget()
    try:
        pkg.matrix.set_match_pair_budget(777)
        assert pkg.matrix.match_pair_budget() == 777
    finally:
        pkg.matrix.set_match_pair_budget(0)
    assert pkg.matrix.match_pair_budget() == default == 1 << 26


@pytest.mark.gpu
def test_match_link_check_on_the_gpu(pkg, tmp_path):
    assert "match abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_match_symbols")
