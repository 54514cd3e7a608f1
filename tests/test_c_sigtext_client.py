"""The entry points of signature JSON written on the device, link-checked from C like the rest of the additive ABI
(tests/test_c_client.py): tests/c_sigtext_symbols.c compiles with -Werror against the headers, links, calls each one."""
import os
import re

import pytest

import test_c_client as base

SYMBOLS = {"smh_index_sigtext", "smh_sigtext_len", "smh_sigtext_documents", "smh_sigtext_doc_offsets", "smh_sigtext_dev", "smh_sigtext_read",
           "smh_sigtext_free", "smh_index_md5", "smh_sigtext_geometry"}


def test_sigtext_symbols_are_declared_exported_and_link_checked(pkg, tmp_path):
    header = open(os.path.join(base.ROOT, "include", "sourmash_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(smh_sigtext_[a-z0-9_]*|smh_index_sigtext|smh_index_md5)\(", code))
    assert declared == SYMBOLS
    ctext = open(os.path.join(base.ROOT, "tests", "c_sigtext_symbols.c")).read()
    assert not [sym for sym in SYMBOLS if not re.search(r"\b%s\(" % sym, ctext)]
    assert SYMBOLS <= set(pkg.exported_symbols())
    assert "sigtext abi client ok" in base._build_and_run(pkg, tmp_path, "c_sigtext_symbols")


@pytest.mark.gpu
def test_sigtext_two_node_text_through_plain_c(pkg, tmp_path):
    assert "sigtext abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_sigtext_symbols")
