"""The clustering rules (include/sourmash_amd.h, smh_index_cluster) on the plain-Python restatement alone: hand-made graphs
whose answers can be read off, and the committed 100-sketch fixture, whose figures DESIGN.md 3.17 quotes.  No device."""
import pytest

import cluster_restatement as CR


def graph_of(n, edges):
    """adj of the undirected edges (u, v, value): common is not looked at by these tests"""
    adj = [dict() for _ in range(n)]
    for e in edges:
        u, v, value = e if len(e) == 3 else (e[0], e[1], 0.5)
        adj[u][v] = adj[v][u] = (value, 1)
    return adj


def test_path_chains_under_components_and_not_under_greedy():
    adj = graph_of(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    scores = [5, 4, 3, 2, 1]
    assert CR.components(adj, scores) == ([0] * 5, [0] * 5, 1)
    # 0 represents and takes 1; 2 sees no representative and represents, takes 3; 4 is left alone
    cluster, rep, _, k = CR.greedy(adj, scores, [1] * 5)
    assert (cluster, rep, k) == ([0, 0, 1, 1, 2], [0, 0, 2, 2, 4], 3)
    reps, rounds = CR.greedy_rounds(adj, scores)
    assert reps == {0, 2, 4} == CR.greedy_representatives(adj, scores) and rounds == 5


def test_star():
    adj = graph_of(6, [(3, v) for v in (0, 1, 2, 4, 5)])
    hub_first = [1, 1, 1, 9, 1, 1]
    assert CR.components(adj, hub_first) == ([0] * 6, [3] * 6, 1)
    assert CR.greedy(adj, hub_first, [1] * 6)[:2] == ([0] * 6, [3] * 6)
    assert CR.greedy_rounds(adj, hub_first) == ({3}, 2)
    hub_last = [5, 5, 5, 0, 5, 5]
    # every leaf represents itself; the hub joins the one first in priority among equal values: the lowest node
    cluster, rep, _, k = CR.greedy(adj, hub_last, [1] * 6)
    assert (cluster, rep, k) == ([0, 1, 2, 0, 3, 4], [0, 1, 2, 0, 4, 5], 5)
    assert CR.components(adj, hub_last) == ([0] * 6, [0] * 6, 1)


def test_two_triangles_joined_by_one_edge():
    adj = graph_of(6, [(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (2, 3)])
    scores = [6, 5, 4, 3, 2, 1]
    assert CR.components(adj, scores) == ([0] * 6, [0] * 6, 1)
    # 0 takes its triangle; 3 is adjacent to the member 2 only, so it represents the other: the bridge does not chain
    cluster, rep, _, k = CR.greedy(adj, scores, [1] * 6)
    assert (cluster, rep, k) == ([0, 0, 0, 1, 1, 1], [0, 0, 0, 3, 3, 3], 2)
    # the bridge's far end first: 3 takes 2, 4 and 5; 0 and 1 are left, 0 takes 1
    cluster, rep, _, k = CR.greedy(adj, [3, 2, 1, 9, 1, 1], [1] * 6)
    assert (cluster, rep, k) == ([0, 0, 1, 1, 1, 1], [0, 0, 3, 3, 3, 3], 2)


def test_ties_and_values():
    # equal scores: the lower node comes first
    adj = graph_of(3, [(0, 1), (1, 2)])
    assert CR.priority([7, 7, 7]) == [0, 1, 2] and CR.priority([1, 7, 7]) == [1, 2, 0]
    assert CR.greedy(adj, [7, 7, 7], [1] * 3)[:2] == ([0, 0, 1], [0, 0, 2])
    assert CR.components(adj, [1, 7, 7])[1] == [1, 1, 1]
    # a member joins the representative with the greatest value, not the first in priority ...
    adj = graph_of(3, [(0, 1, 0.2), (1, 2, 0.9)])
    assert CR.greedy(adj, [9, 1, 8], [1] * 3)[:2] == ([0, 1, 1], [0, 2, 2])
    # ... which may come later than the member in priority only when the member was taken by an earlier one
    adj = graph_of(4, [(0, 1, 0.2), (1, 2, 0.9), (2, 3, 0.1)])
    assert CR.greedy_representatives(adj, [9, 8, 7, 1]) == {0, 2}
    assert CR.greedy(adj, [9, 8, 7, 1], [1] * 4)[1] == [0, 2, 2, 2]
    # isolated nodes are their own clusters, numbered by node
    assert CR.components(graph_of(3, []), [1, 2, 3]) == ([0, 1, 2], [0, 1, 2], 3)
    assert CR.greedy_rounds(graph_of(3, []), [1, 2, 3]) == ({0, 1, 2}, 1)
    with pytest.raises(ValueError):
        CR.graph([[1]], 1, 0.0)                      # a directed containment


def test_descending_path_needs_one_round_per_node():
    n = 70
    adj = graph_of(n, [(v, v + 1) for v in range(n - 1)])
    reps, rounds = CR.greedy_rounds(adj, list(range(n, 0, -1)))
    assert rounds == n and reps == set(range(0, n, 2))


FIGURES = {(CR.JACCARD, 0.0): (2, [99, 1], 13, 5), (CR.MAX_CONTAINMENT, 0.01): (40, None, 46, 5)}


@pytest.mark.parametrize("metric,threshold", sorted(FIGURES))
def test_fixture_figures(sbt_subset_sketches, metric, threshold):
    mins = [s["mins"] for s in sbt_subset_sketches]
    sizes = [len(m) for m in mins]
    adj = CR.graph(mins, metric, threshold)
    n_components, shape, n_reps, n_rounds = FIGURES[(metric, threshold)]
    cluster, rep, k = CR.components(adj, sizes)
    counts = sorted((cluster.count(c) for c in range(k)), reverse=True)
    assert k == n_components
    if shape:
        assert counts == shape
    else:
        assert counts[0] == 26 and counts.count(1) == 32
    reps = CR.greedy_representatives(adj, sizes)
    by_rounds, rounds = CR.greedy_rounds(adj, sizes)
    assert len(reps) == n_reps and by_rounds == reps and rounds == n_rounds
    # independent: no two representatives are adjacent; dominating: everybody else is adjacent to one
    assert not [(u, v) for u in reps for v in adj[u] if v in reps]
    assert not [v for v in range(len(mins)) if v not in reps and not any(u in reps for u in adj[v])]
    g_cluster, g_rep, g_common, g_k = CR.greedy(adj, sizes, sizes)
    assert g_k == n_reps and set(g_rep) == reps
    for v in range(len(mins)):
        assert g_rep[v] == v and g_common[v] == sizes[v] or g_rep[v] in adj[v] and g_common[v] == adj[v][g_rep[v]][1]
    # a component's representative is its member with the most hashes, the lowest node among equals
    for c in range(k):
        members = [v for v in range(len(mins)) if cluster[v] == c]
        assert {rep[v] for v in members} == {min(members, key=lambda v: (-sizes[v], v))}
    if metric == CR.JACCARD:
        assert sum(len(a) for a in adj) == 2 * 1398   # the directed pairs the pair-budget test stands on
