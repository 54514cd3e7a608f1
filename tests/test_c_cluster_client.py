"""The clustering entry points, link-checked from C like the rest of the additive ABI (tests/test_c_client.py):
tests/c_cluster_symbols.c compiles with -Werror against the headers, links, calls each one."""
import os
import re

import pytest

import test_c_client as base

SYMBOLS = {"smh_index_cluster", "smh_cluster_set_pair_budget", "smh_cluster_pair_budget", "smh_cluster_set_rounds", "smh_cluster_rounds",
           "smh_cluster_geometry", "smh_index_sizes"}


def test_cluster_symbols_are_declared_exported_and_link_checked(pkg, tmp_path):
    header = open(os.path.join(base.ROOT, "include", "sourmash_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(smh_[a-z0-9_]*cluster[a-z0-9_]*|smh_index_sizes)\(", code))
    assert declared == SYMBOLS
    assert "SMH_CLUSTER_COMPONENTS = 0" in header and "SMH_CLUSTER_GREEDY = 1" in header
    ctext = open(os.path.join(base.ROOT, "tests", "c_cluster_symbols.c")).read()
    assert not [sym for sym in SYMBOLS if not re.search(r"\b%s\(" % sym, ctext)]
    assert SYMBOLS <= set(pkg.exported_symbols())
    assert "cluster abi client ok" in base._build_and_run(pkg, tmp_path, "c_cluster_symbols")


@pytest.mark.gpu
def test_cluster_four_node_answer_through_plain_c(pkg, tmp_path):
    assert "cluster abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_cluster_symbols")
