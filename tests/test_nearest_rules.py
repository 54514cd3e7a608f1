"""The restatement of the nearest neighbours (tests/nearest_restatement.py) against cases written out by hand: the order, the
tie rule and the cut are what the device kernels are then held to."""
import nearest_restatement as NR
import search_many_restatement as SR


def test_equal_doubles_tie_and_the_node_decides():
    # containment_node of query {1, 2}: node 0 = 1/2, node 1 = 2/4, node 2 = 1/2 again, node 3 = 2/3
    sketches = [[1, 10], [1, 2, 11, 12], [2, 20], [1, 2, 30]]
    got = NR.nearest(sketches, [[1, 2]], 4, SR.CONTAINMENT_NODE, 0.0)
    assert got == [[(3, 2, 3, 2), (0, 1, 2, 2), (1, 2, 4, 2), (2, 1, 2, 2)]]
    assert SR.value(SR.CONTAINMENT_NODE, 1, 2, 2) == SR.value(SR.CONTAINMENT_NODE, 2, 2, 4) == 0.5
    # the same nodes in another order: the tie group follows the nodes, not the fractions
    assert [r[0] for r in NR.nearest(sketches[::-1], [[1, 2]], 4, SR.CONTAINMENT_NODE, 0.0)[0]] == [0, 1, 2, 3]


def test_a_cut_through_a_tie_group():
    sketches = [[1, 10], [1, 2, 11, 12], [2, 20], [1, 2, 30]]
    for k, nodes in ((1, [3]), (2, [3, 0]), (3, [3, 0, 1]), (4, [3, 0, 1, 2])):
        assert [r[0] for r in NR.nearest(sketches, [[1, 2]], k, SR.CONTAINMENT_NODE, 0.0)[0]] == nodes


def test_k_larger_than_the_rows():
    sketches = [[1, 2], [2, 3], [9]]
    got = NR.nearest(sketches, [[2], [9, 1], [7], []], 100, SR.JACCARD, 0.0)
    assert got == [[(0, 1, 2, 1), (1, 1, 2, 1)], [(2, 1, 1, 2), (0, 1, 2, 2)], [], []]
    # the threshold and the count select before the order does
    assert NR.nearest(sketches, [[9, 1]], 100, SR.JACCARD, 0.4) == [[(2, 1, 1, 2)]]
    assert NR.nearest(sketches, [[1, 2, 3]], 1, SR.CONTAINMENT_QUERY, 0.0, 2) == [[(0, 2, 2, 3)]]


def test_value_one_comes_first():
    sketches = [[1, 2, 3, 4], [1, 2], [1, 2, 3]]
    got = NR.nearest(sketches, [[1, 2, 3]], 3, SR.JACCARD, 0.0)
    assert got == [[(2, 3, 3, 3), (0, 3, 4, 3), (1, 2, 2, 3)]]
    assert SR.value(SR.JACCARD, 3, 3, 3) == 1.0
    # under max_containment all three are 1.0: the nodes ascend
    assert [r[0] for r in NR.nearest(sketches, [[1, 2, 3]], 3, SR.MAX_CONTAINMENT, 0.0)[0]] == [0, 1, 2]


def test_a_pair_that_shares_nothing_is_no_neighbour():
    sketches = [[1, 2], [5, 6], []]
    assert NR.nearest(sketches, [[5, 7]], 3, SR.JACCARD, -1.0) == [[(1, 1, 2, 2)]]
    assert NR.nearest(sketches, [[8]], 3, SR.JACCARD, -1.0) == [[]]


def test_nearest_self_leaves_the_diagonal_out():
    sketches = [[1, 2], [2, 3], [3, 4], [9]]
    got = NR.nearest_self(sketches, 1, SR.JACCARD, 0.0)
    assert got == [[(1, 1, 2, 2)], [(0, 1, 2, 2)], [(1, 1, 2, 2)], []]
    assert [[r[0] for r in rows] for rows in NR.nearest_self(sketches, 2, SR.JACCARD, 0.0)] == [[1], [0, 2], [1], []]


def test_select_is_nearest_over_shared_rows():
    sketches = [[1, 2, 3], [3, 4], [1, 5, 6, 7], [2]]
    queries = [[1, 2, 3, 4], [5], []]
    shared = SR.shared(sketches, queries)
    for metric in SR.METRICS:
        for k in (1, 2, NR.MAX_K):
            for threshold in (-1.0, 0.0, 0.3):
                assert NR.select(shared, k, metric, threshold) == NR.nearest(sketches, queries, k, metric, threshold)
