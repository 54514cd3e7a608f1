"""The entry points that gather a batch of queries, link-checked from C like the rest of the additive ABI
(tests/test_c_client.py): tests/c_gather_many_symbols.c compiles with -Werror against the headers, links, calls each one
and frees the rows with free()."""
import os
import re

import pytest

import test_c_client as base

SYMBOLS = {"smh_index_gather_many", "smh_index_gather_block_dev", "smh_gather_many_set_budget", "smh_gather_many_budget"}


def test_gather_many_symbols_are_declared_exported_and_link_checked(pkg, tmp_path):
    header = open(os.path.join(base.ROOT, "include", "sourmash_amd.h")).read()
    declared = set(re.findall(r"\b(smh_(?:index_)?gather_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == SYMBOLS | {"smh_gather_rounds_per_sync"}
    ctext = open(os.path.join(base.ROOT, "tests", "c_gather_many_symbols.c")).read()
    assert not [sym for sym in SYMBOLS if not re.search(r"\b%s\(" % sym, ctext)]
    assert "free(rows)" in ctext
    assert SYMBOLS <= set(pkg.exported_symbols())
    assert "gather many abi client ok" in base._build_and_run(pkg, tmp_path, "c_gather_many_symbols")


def test_budget_needs_no_device(pkg):
    default = pkg.matrix.gather_many_budget()
    try:
        pkg.matrix.set_gather_many_budget(777)
        assert pkg.matrix.gather_many_budget() == 777
    finally:
        pkg.matrix.set_gather_many_budget(0)
    assert pkg.matrix.gather_many_budget() == default == 1 << 26


@pytest.mark.gpu
def test_gather_many_link_check_on_the_gpu(pkg, tmp_path):
    assert "gather many abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_gather_many_symbols")
