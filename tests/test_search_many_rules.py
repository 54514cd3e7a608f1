"""The rules of the thresholded search of a batch (include/sourmash_amd.h, smh_index_search_many), restated
in search_many_restatement.py and checked without a device: the restatement against the oracle's count_common / compare /
containment on the committed fixture, the strict comparison, threshold_common, the self mode, the chunk cutter (restated
there: the product's is csrc/search_many.cpp, search_many_chunk_end, whose chunks tests/test_gpu_search_many.py counts
against the same rule), and the refusals the library decides before it looks at an index or a device.

The refusals of a num query, of an incompatible query and the naming of the lowest failing query need an index, and an index
needs a device: they are in tests/test_gpu_search_many.py (test_errors_write_nothing)."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import search_many_restatement as SR

SENTINEL = 0xDEADBEEFDEADBEEF


@pytest.fixture(scope="module")
def fixture_case(pyoracle, sbt_subset_sketches):
    """the first 30 sketches of the fixture as oracle sketches, and queries: some of them, a union, a foreign one"""
    def mk(hashes):
        mh = pyoracle.MinHash(0, 21, False, 42, sbt_subset_sketches[0]["max_hash"], False)
        mh.add_many(hashes)
        return mh
    mins = [s["mins"] for s in sbt_subset_sketches[:30]]
    union = sorted(set(mins[3]) | set(mins[4]) | set(mins[17]))
    foreign = [h + 1 for h in union[:200] if h + 1 not in set(union)]
    queries = mins[:6] + [union, foreign, []]
    return mins, [mk(m) for m in mins], queries, [mk(q) for q in queries]


@pytest.mark.parametrize("metric", SR.METRICS)
def test_restatement_against_the_oracle(fixture_case, metric):
    mins, nodes, queries, qsk = fixture_case
    reported = 0
    for threshold in (0.0, 0.1, 1.0):
        got = SR.search_many(mins, queries, metric, threshold)
        for q, rows in enumerate(got):
            exp = []
            for i, node in enumerate(nodes):
                common = node.count_common(qsk[q])
                if common == 0:
                    continue
                lq, ls = len(qsk[q].mins), len(node.mins)
                v = {SR.JACCARD: node.compare(qsk[q]),                        # (scaled sketches: common / union)
                     SR.CONTAINMENT_NODE: node.containment(qsk[q]),
                     SR.CONTAINMENT_QUERY: qsk[q].containment(node),
                     SR.MAX_CONTAINMENT: common / min(lq, ls)}[metric]
                if v > threshold:
                    exp.append((i, common, ls, lq))
            assert rows == exp, (threshold, q)
            reported += len(rows)
        if threshold == 1.0:
            assert all(not rows for rows in got), "no value exceeds 1"
    assert reported > 20
    assert SR.search_many(mins, queries, metric, 0.0)[-1] == [] and SR.search_many([], queries, metric, 0.0) == [[]] * len(queries)


def test_the_comparison_is_strict():
    below = math.nextafter(0.5, 0.0)
    # common 1 of size 2: node {1, 2} against query {1}; its value is 0.5 under JACCARD and CONTAINMENT_NODE
    for metric in (SR.JACCARD, SR.CONTAINMENT_NODE):
        assert SR.search_many([[1, 2]], [[1]], metric, 0.5) == [[]]
        assert SR.search_many([[1, 2]], [[1]], metric, below) == [[(0, 1, 2, 1)]]
    # and from the query's side: query {1, 2} against node {1}
    assert SR.search_many([[1]], [[1, 2]], SR.CONTAINMENT_QUERY, 0.5) == [[]]
    assert SR.search_many([[1]], [[1, 2]], SR.CONTAINMENT_QUERY, below) == [[(0, 1, 1, 2)]]
    # min(|Q|, |S|) = 2: two of {1, 2, 3} against {1, 5}
    assert SR.search_many([[1, 5]], [[1, 2, 3]], SR.MAX_CONTAINMENT, 0.5) == [[]]
    assert SR.search_many([[1, 5]], [[1, 2, 3]], SR.MAX_CONTAINMENT, below) == [[(0, 1, 2, 3)]]
    # a pair that shares nothing is never reported, whatever the threshold is; the value 1 never exceeds 1
    for metric in SR.METRICS:
        assert SR.search_many([[1, 2], []], [[3], []], metric, -1.0) == [[], []]
        assert SR.search_many([[1, 2]], [[1, 2]], metric, 1.0) == [[]]
        assert SR.search_many([[1, 2]], [[1, 2]], metric, -math.inf) == [[(0, 2, 2, 2)]]
        assert SR.search_many([[1, 2]], [[1, 2]], metric, math.inf) == [[]]


def test_threshold_common_zero_is_read_as_one():
    rng = random.Random(5)
    pool = rng.sample(range(1, 1 << 40), 120)
    sketches = [rng.sample(pool, rng.randint(0, 40)) for _ in range(14)]
    queries = [rng.sample(pool, k) for k in (0, 3, 30, 120)]
    for metric in SR.METRICS:
        assert SR.search_many(sketches, queries, metric, 0.0, 0) == SR.search_many(sketches, queries, metric, 0.0, 1)
        few = SR.search_many(sketches, queries, metric, 0.0, 5)
        assert few == [[r for r in rows if r[1] >= 5] for rows in SR.search_many(sketches, queries, metric, 0.0, 0)]
        assert 0 < sum(map(len, few)) < sum(map(len, SR.search_many(sketches, queries, metric, 0.0, 0)))


def test_self_mode_is_the_general_mode_minus_the_diagonal_and_the_lower_rows():
    rng = random.Random(8)
    pool = rng.sample(range(1, 1 << 40), 90)
    sketches = [rng.sample(pool, rng.randint(0, 30)) for _ in range(12)] + [[]]
    sketches.append(list(sketches[2]))                                     # a duplicate is not the diagonal
    for metric in SR.METRICS:
        full = SR.search_many(sketches, sketches, metric, 0.05)
        both = SR.search_self(sketches, metric, 0.05)
        upper = SR.search_self(sketches, metric, 0.05, upper_only=True)
        for q in range(len(sketches)):
            assert both[q] == [r for r in full[q] if r[0] != q]
            assert upper[q] == [r for r in full[q] if r[0] > q]
            assert (q, len(sketches[q]), len(sketches[q]), len(sketches[q])) in full[q] or not sketches[q]
        assert (13, len(sketches[2]), len(sketches[2]), len(sketches[2])) in upper[2]
        if metric in (SR.JACCARD, SR.MAX_CONTAINMENT):                     # the symmetric metrics: the lower rows mirror the upper
            assert sum(map(len, both)) == 2 * sum(map(len, upper))
            assert {(q, r[0]) for q in range(len(sketches)) for r in both[q]} == \
                {p for q in range(len(sketches)) for r in upper[q] for p in ((q, r[0]), (r[0], q))}


@pytest.mark.parametrize("n,nq", [(50, 9), (1, 7), (7, 1), (3, 20)])
def test_chunk_cutter(n, nq):
    sizes = [10 * (k % 4) for k in range(nq)]                 # empty queries among them
    for budget in (1, n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1, nq * n, 1 << 26):
        chunks = SR.cut_chunks(sizes, n, max(budget, 1))
        assert chunks[0][0] == 0 and chunks[-1][1] == nq
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))      # no query split, none left out
        assert all(b > a for a, b in chunks)                              # no chunk empty
        assert all((b - a) * n <= budget or b - a == 1 for a, b in chunks)
        assert len(chunks) == -(-nq // max(budget // n, 1))               # as few chunks as the rule allows
    if (n, nq) == (50, 9):
        assert [len(SR.cut_chunks(sizes, n, b)) for b in (49, 50, 100, 101, 449, 450, 1 << 26)] == [9, 9, 5, 5, 2, 1, 1]


def test_chunk_cutter_limits():
    assert SR.cut_chunks([], 5, 100) == []
    # one grid dimension of queries
    chunks = SR.cut_chunks([1] * 70000, 2, 1 << 26)
    assert [b - a for a, b in chunks] == [65535, 4465]
    # positions: a chunk of several queries stays below 2^32 - 1, a single query may be anything
    big = 3 << 30
    assert SR.cut_chunks([big, big, 5, big], 1, 1 << 26) == [(0, 1), (1, 3), (3, 4)]
    assert SR.cut_chunks([1 << 31, (1 << 31) - 2, 1], 1, 1 << 26) == [(0, 2), (2, 3)]
    # an index without nodes costs no counters
    assert SR.cut_chunks([3, 3], 0, 1) == [(0, 1), (1, 2)]


def test_geometry_and_budget_need_no_device(pkg):
    short_owners, tile, max_queries = pkg.matrix.search_geometry()
    assert 1 <= short_owners < 63 and tile % 64 == 0 and tile >= 64 and max_queries == SR.MAX_QUERIES
    default = pkg.matrix.search_many_budget()
    try:
        pkg.matrix.set_search_many_budget(777)
        assert pkg.matrix.search_many_budget() == 777
    finally:
        pkg.matrix.set_search_many_budget(0)
    assert pkg.matrix.search_many_budget() == default == 1 << 26
    assert [pkg.index.SEARCH_METRICS[k] for k in ("jaccard", "containment_node", "containment_query", "max_containment")] == list(SR.METRICS)


def test_refusals_decided_before_an_index_or_a_device_is_looked_at(pkg):
    """a NaN threshold and an unknown metric (SOURMASH_ERROR_CODE_MSG) and NULL outputs (a panic) from all three entry
    points, with no index at all (these are refused first), and nothing written"""
    L = pkg.lib()
    u64p = C.POINTER(C.c_uint64)
    rowp = C.POINTER(pkg._lib.SmhSearchRow)
    q = pkg.KmerMinHash(0, 21, False, 42, 1 << 60)
    arr = (C.c_void_p * 1)(q._p)
    off = np.zeros(2, dtype=np.uint64)

    def forms(metric, threshold, row_off, rows):
        ro = row_off.ctypes.data_as(u64p) if row_off is not None else None
        yield "many", lambda: L.smh_index_search_many(None, arr, 1, metric, threshold, 0, ro, rows)
        yield "block", lambda: L.smh_index_search_block_dev(None, None, off.ctypes.data_as(u64p), 1, metric, threshold, 0, ro, rows, None)
        yield "self", lambda: L.smh_index_search_self(None, metric, threshold, 0, True, ro, rows)

    def refused(metric, threshold, null_offsets=False, null_rows=False):
        out = []
        for name, fn in forms(metric, threshold, None if null_offsets else row_off, None if null_rows else C.byref(rows_p)):
            with pytest.raises(pkg.SourmashError) as ei:
                pkg.errors.call(fn)
            assert (row_off == SENTINEL).all() and not rows_p, name
            out.append((ei.value.code, ei.value.message))
        return out

    row_off = np.full(2, SENTINEL, dtype=np.uint64)
    rows_p = rowp()
    for rc, text in refused(0, float("nan")):
        assert rc == 3 and "NaN" in text, text
    for metric in (4, 99, 0xFFFFFFFF):
        for rc, text in refused(metric, 0.1):
            assert rc == 3 and "metric" in text, text
    for rc, text in refused(0, 0.1, null_offsets=True):       # (a NULL argument is a panic, as everywhere in the ABI)
        assert rc == 1 and "row_offsets" in text, text
    for rc, text in refused(0, 0.1, null_rows=True):
        assert rc == 1 and "rows" in text, text
    for rc, text in refused(7, float("nan"), null_offsets=True, null_rows=True):
        assert rc == 1 and "row_offsets" in text, text
    # with everything in order the call gets as far as the device (code 2 without one) or the missing index (a panic)
    for rc, text in refused(3, 0.1):
        assert rc in (1, 2) and "NaN" not in text and "metric" not in text, text
    # the Python layer refuses an unknown metric by name
    with pytest.raises(KeyError):
        pkg.index.SEARCH_METRICS["cosine"]


def test_search_result_derives_the_floats_and_ani(pkg):
    rows = np.array([(2, 1, 2, 1), (5, 3, 4, 6)], dtype=pkg.index._SEARCH_ROW)
    res = pkg.index.SearchResult(np.array([0, 1, 1, 2], dtype=np.uint64), rows, ksize=21, molecule="DNA")
    assert len(res) == 2 and res.node.tolist() == [2, 5] and res.query().tolist() == [0, 2]
    assert res.rows_of(0) == slice(0, 1) and res.rows_of(1) == slice(1, 1)
    for k, (node, common, ls, lq) in enumerate(rows.tolist()):
        assert res.jaccard[k] == SR.value(SR.JACCARD, common, lq, ls)
        assert res.containment_node[k] == SR.value(SR.CONTAINMENT_NODE, common, lq, ls)
        assert res.containment_query[k] == SR.value(SR.CONTAINMENT_QUERY, common, lq, ls)
        assert res.max_containment[k] == SR.value(SR.MAX_CONTAINMENT, common, lq, ls)
    # (numpy's pow and Python's may differ in the last place)
    assert res.ani().tolist() == pytest.approx([1.0, 0.5 ** (1.0 / 21)], rel=1e-14)
    assert res.ani("containment_node").tolist() == pytest.approx([0.5 ** (1.0 / 21), 0.75 ** (1.0 / 21)], rel=1e-14)
    with pytest.raises(ValueError):
        res.ani("jaccard")
    for molecule in ("protein", "dayhoff", "hp", None):
        with pytest.raises(ValueError):
            pkg.index.SearchResult(res.offsets, rows, ksize=21, molecule=molecule).ani()
