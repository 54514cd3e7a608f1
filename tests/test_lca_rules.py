"""The rules of the taxonomic LCA (include/sourmash_amd.h, "Taxonomic LCA") on hand-checkable cases, the join fold pinned to
the literal tree rule, the taxonomy's refusals, the host helpers and the getters.  No GPU."""
import collections
import ctypes as C
import random

import numpy as np
import pytest

import lca_restatement as R

NO = R.NO_TAXON

#        0
#      /   \
#     1     2
#    / \     \
#   3   4     5
#   |
#   6
PARENT = [0, 0, 0, 1, 1, 2, 3]


def test_classification_by_hand():
    assert R.find_lca(PARENT, [1, 3, 6]) == (6, R.FOUND), "a chain gives its deepest taxon"
    assert R.find_lca(PARENT, [3, 4]) == (1, R.DISAGREE), "a fork gives the branching point"
    assert R.find_lca(PARENT, [1, 6, 4]) == (1, R.DISAGREE), "an ancestor plus a fork below it"
    assert R.find_lca(PARENT, [3, 6]) == (6, R.FOUND), "not lca(S): the ancestor is on the path"
    assert R.find_lca(PARENT, [6, 5]) == (0, R.DISAGREE)
    assert R.find_lca(PARENT, [0]) == (0, R.FOUND), "root only"
    assert R.find_lca(PARENT, [0, 5]) == (5, R.FOUND)
    assert R.find_lca(PARENT, []) == (NO, R.NONE), "empty"
    assert R.find_lca(PARENT, [4, 4, 4]) == (4, R.FOUND)


def test_lca_and_hash_taxa_by_hand():
    assert R.lca(PARENT, 6, 4) == 1 and R.lca(PARENT, 6, 3) == 3 and R.lca(PARENT, 6, 5) == 0 and R.lca(PARENT, 2, 2) == 2
    assert R.lca(PARENT, NO, 4) == 4 and R.lca(PARENT, 4, NO) == 4 and R.lca(PARENT, NO, NO) == NO
    node_taxon = [6, 4, NO, NO, 5]
    owners = R.owners_of([[10, 20, 30], [20, 30], [30, 40], [40], [30, 50]])
    assert R.hash_taxon(PARENT, node_taxon, owners, 10) == 6
    assert R.hash_taxon(PARENT, node_taxon, owners, 20) == 1
    assert R.hash_taxon(PARENT, node_taxon, owners, 30) == 0, "the owner without a lineage is ignored"
    assert R.hash_taxon(PARENT, node_taxon, owners, 40) == NO, "held only by nodes without a lineage: unassigned"
    assert R.hash_taxon(PARENT, node_taxon, owners, 60) == NO
    pairs, per = R.counts(PARENT, node_taxon, owners, [60, 50, 40, 30, 20, 10, 5])
    assert per == [NO, 6, 1, 0, NO, 5, NO] and pairs == [(0, 1), (1, 1), (5, 1), (6, 1)]
    assert R.rollup(PARENT, pairs) == {0: 4, 1: 2, 3: 1, 6: 1, 2: 1, 5: 1}
    assert R.classify_counts(PARENT, [(6, 3), (4, 1), (5, 2)], 2) == (0, R.DISAGREE)
    assert R.classify_counts(PARENT, [(6, 3), (4, 1), (5, 2)], 3) == (6, R.FOUND)
    assert R.classify_counts(PARENT, [(6, 3), (4, 1), (5, 2)], 4) == (NO, R.NONE)


def random_taxonomy(rng, n):
    """shapes from a chain to a star"""
    reach = rng.choice([1, 2, 5, n])
    return [0] + [rng.randrange(max(0, t - reach), t) for t in range(1, n)]


def fold(parent, summaries, rng):
    """merges the summaries in random order and random grouping until one is left"""
    items = list(summaries)
    rng.shuffle(items)
    while len(items) > 1:
        i = rng.randrange(len(items) - 1)
        j = rng.randrange(i + 1, len(items))
        b = items.pop(j)
        a = items.pop(i)
        items.insert(rng.randrange(len(items) + 1), R.join(parent, a, b) if rng.random() < 0.5 else R.join(parent, b, a))
    return items[0] if items else None


def test_the_join_fold_equals_the_literal_rule():
    rng = random.Random(2024)
    statuses = collections.Counter()
    for trial in range(3000):
        n = rng.choice([1, 2, 3, 8, 30])
        parent = random_taxonomy(rng, n)
        taxa = [rng.randrange(n) for _ in range(rng.choice([0, 1, 2, 3, 5, 12]))]
        want = R.find_lca(parent, taxa)
        summaries = [(t, False) for t in taxa] + [None] * rng.randrange(3)   # (the identity may appear anywhere)
        got = R.status_of(fold(parent, summaries, rng))
        assert got == want, (parent, taxa)
        statuses[want[1]] += 1
    assert min(statuses[R.NONE], statuses[R.FOUND], statuses[R.DISAGREE]) > 100


def test_host_helpers_equal_the_restatement(pkg):
    rng = random.Random(7)
    for trial in range(300):
        n = rng.choice([1, 2, 6, 25])
        parent = random_taxonomy(rng, n)
        taxa = sorted(rng.sample(range(n), rng.randrange(0, min(n, 6) + 1)))
        cnt = [rng.randrange(1, 5) for _ in taxa]
        pairs = list(zip(taxa, cnt))
        t, c = np.array(taxa, dtype=np.uint32), np.array(cnt, dtype=np.uint64)
        assert pkg.index.lca_summarize(np.array(parent, dtype=np.uint32), t, c) == R.rollup(parent, pairs)
        for thr in (1, 2, 3, 9):
            assert pkg.index.lca_classify(parent, t, c, thr) == R.classify_counts(parent, pairs, thr), (parent, pairs, thr)
    assert (pkg.index.NO_TAXON, pkg.index.LCA_NONE, pkg.index.LCA_FOUND, pkg.index.LCA_DISAGREE) == (NO, R.NONE, R.FOUND, R.DISAGREE)


def check_taxonomy(pkg, parent, node_taxon, index_len):
    p = np.array(parent, dtype=np.uint32)
    t = np.array(node_taxon, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    try:
        rc = pkg.errors.call(pkg.lib().smh_lca_check_taxonomy, p.ctypes.data_as(u32p), len(p), t.ctypes.data_as(u32p), len(t), index_len)
    except pkg.SourmashError as e:
        return e
    assert rc == 0
    return None


def test_the_refusals_of_a_taxonomy_name_the_entry(pkg):
    assert check_taxonomy(pkg, PARENT, [6, NO, 0], 3) is None
    assert check_taxonomy(pkg, [0], [], 0) is None
    cases = [((PARENT, [6, NO, 0], 4), "n_nodes is 3 but the index holds 4"),
             (([1, 0, 0], [0], 1), "parent[0] is 1"),
             (([0, 0, 2, 1], [0], 1), "parent[2] is 2"),
             (([0, 0, 1, 5, 1], [0], 1), "parent[3] is 5"),
             ((PARENT, [6, NO, 7], 3), "node_taxon[2] is 7"),
             (([], [0], 1), "n_taxa is 0")]
    for args, words in cases:
        e = check_taxonomy(pkg, *args)
        assert e is not None and e.code == 3 and e.message.startswith("lca: ") and words in e.message, (args, e and e.message)
    assert check_taxonomy(pkg, PARENT, [0, 0, 0], 3) is None, "a refusal leaves the library usable"


def test_geometry_and_budget_need_no_device(pkg):
    owner_lane_max, record_lane_max, threads = pkg.matrix.lca_geometry()
    assert 1 <= owner_lane_max < 63 and 1 <= record_lane_max < 63 and threads == 64
    default = pkg.matrix.lca_budget()
    try:
        pkg.matrix.set_lca_budget(777)
        assert pkg.matrix.lca_budget() == 777
    finally:
        pkg.matrix.set_lca_budget(0)
    assert pkg.matrix.lca_budget() == default == 1 << 26
    assert pkg.lib().smh_index_has_taxonomy(None) is False
