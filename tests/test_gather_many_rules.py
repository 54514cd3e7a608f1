"""The rules of gather for a batch of queries (include/sourmash_amd.h, smh_index_gather_many), restated with
gather_restatement.py and checked without a device: the batch is a loop, the per-query row bound that sizes the device rows,
and the chunk cutter (restated here: the product's is csrc/gather_many.cpp, gather_many_chunk_end, whose chunk counts
tests/test_gpu_gather_many.py checks against this same rule)."""
import random

import pytest

import gather_restatement as GR

MAX_QUERIES = 65535            # queries per chunk: the second dimension of a grid
MAX_POSITIONS = 0xFFFFFFFF     # a chunk of several queries holds fewer positions than this


def gather_many(sketches, queries, abunds=None, threshold=0, capacity=None):
    """the batch, restated: one GR.gather per query, nothing shared"""
    abunds = abunds or [None] * len(queries)
    return [GR.gather(sketches, q, a, threshold, capacity) for q, a in zip(queries, abunds)]


def row_bound(sketches, query, threshold, capacity):
    """what sizes a query's rows on the device: min(capacity, sketches that reach the threshold at the start)"""
    threshold = max(1, threshold)
    reach = sum(1 for s in sketches if len(set(s) & set(query)) >= threshold)
    return reach if capacity is None else min(capacity, reach)


def cut_chunks(sizes, n_nodes, budget):
    """[(first query, end)]: as many consecutive queries as the budget holds (query, node) counters for, one at least, at most
    MAX_QUERIES, and fewer than MAX_POSITIONS positions unless the chunk is a single query"""
    per = min(max(budget // max(n_nodes, 1), 1), MAX_QUERIES)
    out, a = [], 0
    while a < len(sizes):
        b = min(len(sizes), a + per)
        while b > a + 1 and sum(sizes[a:b]) >= MAX_POSITIONS:
            b -= 1
        out.append((a, b))
        a = b
    return out


def random_case(rng, n, universe, lo, hi):
    pool = rng.sample(range(1, 1 << 40), universe)
    sketches = [rng.sample(pool, rng.randint(lo, hi)) for _ in range(n)]
    return pool, sketches


def test_a_batch_is_a_loop_and_queries_do_not_interact():
    rng = random.Random(4)
    pool, sketches = random_case(rng, 12, 300, 0, 60)
    queries = [rng.sample(pool, k) for k in (0, 1, 40, 150, 300)] + [[(1 << 50) + i for i in range(5)]]
    abunds = [{h: rng.randint(1, 9) for h in q} if k % 2 else None for k, q in enumerate(queries)]
    for thr, cap in ((0, None), (3, None), (1, 2), (5, 0)):
        batch = gather_many(sketches, queries, abunds, thr, cap)
        twice = gather_many(sketches, queries + queries, abunds + abunds, thr, cap)
        assert twice == batch + batch
        back = gather_many(sketches, queries[::-1], abunds[::-1], thr, cap)
        assert back == batch[::-1]
        for (rows, assigned), q in zip(batch, queries):
            assert len(assigned) == len(set(q))
            assert sorted(a for a in set(assigned) if a != GR.UNASSIGNED) == list(range(len(rows)))
    assert gather_many(sketches, []) == []
    assert gather_many([], queries[:3]) == [([], [GR.UNASSIGNED] * len(q)) for q in queries[:3]]


@pytest.mark.parametrize("seed", range(6))
def test_row_bound_holds(seed):
    rng = random.Random(seed)
    pool, sketches = random_case(rng, 15, 200, 0, 50)
    sketches += [list(sketches[0]), []]                       # a duplicate never wins; an empty sketch never reaches 1
    for k in (0, 5, 60, 200):
        q = rng.sample(pool, k)
        for thr in (0, 1, 4, 12):
            for cap in (None, 0, 3, 100):
                rows, _ = GR.gather(sketches, q, None, thr, cap)
                assert len(rows) <= row_bound(sketches, q, thr, cap), (k, thr, cap)
                # every winner reached the threshold at the start, and wins once
                assert len({r["match"] for r in rows}) == len(rows)
                assert all(r["common_original"] >= r["common_remaining"] >= max(1, thr) for r in rows)


def test_row_bound_is_tight():
    # disjoint sketches: every one that reaches the threshold wins exactly once
    sketches = [list(range(100 * i, 100 * i + 3 + i)) for i in range(10)]
    query = [h for s in sketches for h in s]
    for thr, cap in ((0, None), (6, None), (6, 3), (13, None), (1, 10), (1, 11)):
        rows, _ = GR.gather(sketches, query, None, thr, cap)
        assert len(rows) == row_bound(sketches, query, thr, cap), (thr, cap)
    assert row_bound(sketches, query, 6, None) == 7 and row_bound(sketches, query, 13, None) == 0
    # and it is only a bound: a duplicate reaches the threshold but has nothing left when its turn would come
    rows, _ = GR.gather(sketches + [list(sketches[9])], query, None, 1)
    assert len(rows) == 10 and row_bound(sketches + [list(sketches[9])], query, 1, None) == 11


@pytest.mark.parametrize("n,nq", [(50, 9), (1, 7), (7, 1), (3, 20)])
def test_chunk_cutter(n, nq):
    sizes = [10 * (k % 4) for k in range(nq)]                 # empty queries among them
    for budget in (1, n, n + 1, 2 * n - 1, 2 * n, nq * n, 1 << 26):
        chunks = cut_chunks(sizes, n, budget)
        assert chunks[0][0] == 0 and chunks[-1][1] == nq
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))      # no query split, none left out
        assert all(b > a for a, b in chunks)                              # no chunk empty
        assert all((b - a) * n <= budget or b - a == 1 for a, b in chunks)
        # as few chunks as the rule allows
        per = max(budget // n, 1)
        assert len(chunks) == -(-nq // per)
    if (n, nq) == (50, 9):
        assert [len(cut_chunks(sizes, n, b)) for b in (1, 50, 51, 100, 449, 450, 1 << 26)] == [9, 9, 9, 5, 2, 1, 1]


def test_chunk_cutter_limits():
    assert cut_chunks([], 5, 100) == []
    # the grid's second dimension
    chunks = cut_chunks([1] * 70000, 1, 1 << 26)
    assert [b - a for a, b in chunks] == [65535, 4465]
    # positions: a chunk of several queries stays below 2^32 - 1, a single query may be anything
    big = 3 << 30
    assert cut_chunks([big, big, 5, big], 1, 1 << 26) == [(0, 1), (1, 3), (3, 4)]
    assert cut_chunks([1 << 31, (1 << 31) - 2, 1], 1, 1 << 26) == [(0, 2), (2, 3)]
    # an index without nodes costs no counters
    assert cut_chunks([3, 3], 0, 1) == [(0, 1), (1, 2)]
