"""The nearest-neighbour entry points, link-checked from C like the rest of the additive ABI (tests/test_c_client.py):
tests/c_nearest_symbols.c compiles with -Werror against the headers, links, calls each one."""
import os
import re

import pytest

import test_c_client as base

SYMBOLS = {"smh_index_nearest_many", "smh_index_nearest_block_dev", "smh_index_nearest_self", "smh_nearest_geometry"}


def test_nearest_symbols_are_declared_exported_and_link_checked(pkg, tmp_path):
    header = open(os.path.join(base.ROOT, "include", "sourmash_amd.h")).read()
    declared = set(re.findall(r"\b(smh_[a-z0-9_]*nearest[a-z0-9_]*)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == SYMBOLS
    ctext = open(os.path.join(base.ROOT, "tests", "c_nearest_symbols.c")).read()
    assert not [sym for sym in SYMBOLS if not re.search(r"\b%s\(" % sym, ctext)]
    assert SYMBOLS <= set(pkg.exported_symbols())
    assert "nearest abi client ok" in base._build_and_run(pkg, tmp_path, "c_nearest_symbols")


def test_k_is_refused_without_a_device(pkg):
    """k == 0 and k > max_k are MSG, the message names the limit, and nothing is written -- decided before the device"""
    import ctypes as C
    import numpy as np
    L = pkg.lib()
    max_k, tile, slots = pkg.matrix.nearest_geometry()
    assert max_k >= 100 and tile == pkg.matrix.search_geometry()[1] and slots > max_k
    for k in (0, max_k + 1, 0xFFFFFFFF):
        roff = np.full(2, 7, dtype=np.uint64)
        rows_p = C.POINTER(pkg._lib.SmhSearchRow)()
        L.sourmash_err_clear()
        rc = L.smh_index_nearest_self(None, k, 0, 0.0, 0, roff.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(rows_p))
        assert rc == 3 and not rows_p and roff.tolist() == [7, 7]
        with pytest.raises(pkg.SourmashError) as ei:
            pkg.errors.check()
        assert ei.value.code == 3 and str(max_k) in ei.value.message and "k" in ei.value.message
    # a NaN threshold and an unknown metric are looked at first, as search_many looks at them
    for k, metric, threshold in ((0, 9, 0.0), (0, 0, float("nan"))):
        L.sourmash_err_clear()
        roff = np.full(2, 7, dtype=np.uint64)
        rows_p = C.POINTER(pkg._lib.SmhSearchRow)()
        assert L.smh_index_nearest_self(None, k, metric, threshold, 0, roff.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(rows_p)) == 3
        with pytest.raises(pkg.SourmashError) as ei:
            pkg.errors.check()
        assert "search_many" in ei.value.message and roff.tolist() == [7, 7]


@pytest.mark.gpu
def test_nearest_four_node_answer_through_plain_c(pkg, tmp_path):
    assert "nearest abi client ok (gpu)" in base._build_and_run(pkg, tmp_path, "c_nearest_symbols")
