"""Clustering a resident index on the device (smh_index_cluster; ResidentIndex.cluster) against the plain-Python restatement:
every output is an integer, so the arrays must be EQUAL.  ResidentIndex.pairwise (the rows the clusters are made of) is the
second witness.  The shapes stand on both sides of the sizes smh_cluster_geometry reports."""
import ctypes as C
import math

import numpy as np
import pytest

import cluster_restatement as CR

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
SENTINEL = 0xDEADBEEF
NAMES = {CR.JACCARD: "jaccard", CR.MAX_CONTAINMENT: "max_containment"}
LINKS = {CR.COMPONENTS: "components", CR.GREEDY: "greedy"}


def mk(pkg, hashes, abunds=None, max_hash=M64, ksize=21, seed=42, protein=False, num=0):
    """a sketch holding `hashes`; abunds ({hash: abundance}) makes it track abundances"""
    mh = pkg.KmerMinHash(num, ksize, protein, seed, max_hash, abunds is not None)
    h = sorted(int(x) for x in hashes)
    if abunds is not None and h:
        mh.add_many_with_abund([(x, abunds[x]) for x in h])
    elif h:
        mh.add_many(np.array(h, dtype=np.uint64))
    return mh


def as_lists(res):
    """a Clustering as the restatement writes it"""
    assert res.cluster.dtype == np.uint32 and res.representative.dtype == np.uint32
    return (res.cluster.tolist(), res.representative.tolist(), None if res.rep_common is None else res.rep_common.tolist(), res.n_clusters)


def check(pkg, sketches, metric=CR.JACCARD, threshold=0.0, threshold_common=0, linkage=CR.COMPONENTS, scores=None, index=None):
    index = index or pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    res = index.cluster(threshold, NAMES[metric], LINKS[linkage], scores=scores, threshold_bp=threshold_common, scaled=1)
    got = as_lists(res)
    assert got == CR.cluster(sketches, metric, threshold, threshold_common, linkage, scores)
    assert res.sizes().sum() == len(sketches) and len(res.sizes()) == res.n_clusters
    return got


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


def edge_sketches(n, edges):
    """n sketches of a handful of hashes: node v alone holds 10 v + 1 .. 10 v + 3, an edge e is one more hash that its two ends
    hold -- so two adjacent nodes of degree 1 have Jaccard 1 / 7"""
    out = [[10 * v + 1, 10 * v + 2, 10 * v + 3] for v in range(n)]
    for k, (u, v) in enumerate(edges):
        out[u].append((1 << 40) + k)
        out[v].append((1 << 40) + k)
    return out


@pytest.fixture(scope="module")
def geometry(pkg):
    lane_max, tile = pkg.matrix.cluster_geometry()
    assert 1 <= lane_max < 3000 and tile == pkg.matrix.search_geometry()[1]
    return lane_max, tile


# ---------------------------------------------------------------------------------- the committed fixture

class Fixture:
    def __init__(self, pkg, sketches):
        self.mins = [s["mins"] for s in sketches]
        self.max_hash = sketches[0]["max_hash"]
        self.index = pkg.index.ResidentIndex([mk(pkg, m, dict(zip(m, s["abundances"])), max_hash=self.max_hash)
                                              for m, s in zip(self.mins, sketches)])
        self.sizes = [len(m) for m in self.mins]
        self.graphs = {}

    def graph(self, metric, threshold):                     # once per rule: both linkages read it
        key = (metric, threshold)
        if key not in self.graphs:
            self.graphs[key] = CR.graph(self.mins, metric, threshold)
        return self.graphs[key]


@pytest.fixture(scope="module")
def fx(pkg, sbt_subset_sketches):
    return Fixture(pkg, sbt_subset_sketches)


@pytest.mark.parametrize("metric", [CR.JACCARD, CR.MAX_CONTAINMENT])
@pytest.mark.parametrize("threshold", [0.0, 0.01, 0.1, 1.0])
def test_fixture(fx, metric, threshold):
    adj = fx.graph(metric, threshold)
    comp = as_lists(fx.index.cluster(threshold, NAMES[metric], "components"))
    assert comp == CR.components(adj, fx.sizes)[:2] + (None, CR.components(adj, fx.sizes)[2])
    res = fx.index.cluster(threshold, NAMES[metric], "greedy")
    assert as_lists(res) == CR.greedy(adj, fx.sizes, fx.sizes)
    if threshold == 1.0:                                     # above every value: n singletons
        assert comp[0] == comp[1] == list(range(100)) and comp[3] == 100 and res.n_clusters == 100
    if (metric, threshold) in ((CR.JACCARD, 0.0), (CR.MAX_CONTAINMENT, 0.01)):
        assert (comp[3], res.n_clusters) == {CR.JACCARD: (2, 13), CR.MAX_CONTAINMENT: (40, 46)}[metric]
    # the value derived on the host is the rule's own double
    for v in range(100):
        r = int(res.representative[v])
        assert res.rep_value[v] == (1.0 if r == v else adj[v][r][0])


@pytest.mark.parametrize("metric", [CR.JACCARD, CR.MAX_CONTAINMENT])
def test_second_witnesses(fx, metric):
    """components == a union-find over pairwise(upper=True)'s rows; greedy rep_common == the common of the pairwise row"""
    threshold = 0.01
    rows = fx.index.pairwise(threshold, NAMES[metric], upper=True)
    parent = list(range(100))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for q, i in zip(rows.query().tolist(), rows.node.tolist()):
        a, b = find(q), find(i)
        if a != b:
            parent[max(a, b)] = min(a, b)
    roots = sorted({find(v) for v in range(100)})
    res = fx.index.cluster(threshold, NAMES[metric], "components")
    assert res.cluster.tolist() == [roots.index(find(v)) for v in range(100)] and res.n_clusters == len(roots)
    assert [res.members(c)[0] for c in range(res.n_clusters)] == roots
    full = fx.index.pairwise(threshold, NAMES[metric], upper=False)
    common = {(q, i): c for q, i, c in zip(full.query().tolist(), full.node.tolist(), full.common.tolist())}
    g = fx.index.cluster(threshold, NAMES[metric], "greedy")
    members = 0
    for v in range(100):
        r = int(g.representative[v])
        if r != v:
            members += 1
            assert g.rep_common[v] == common[(v, r)]
        else:
            assert g.rep_common[v] == fx.sizes[v]
    assert members == 100 - g.n_clusters > 20


# ---------------------------------------------------------------------------------- the order of the unions

def test_order_independence(pkg):
    n = 200
    perm = [(k * 73 + 11) % n for k in range(n)]            # a fixed permutation: place k of the path is node perm[k]
    for place, node in ((0, 0), (n - 1, 1), (n // 2, 2)):   # small ids at both ends and in the middle
        j = perm.index(node)
        perm[j], perm[place] = perm[place], perm[j]
    assert sorted(perm) == list(range(n)) and (perm[0], perm[n - 1], perm[n // 2]) == (0, 1, 2)
    results = []
    for order in (perm, [n - 1 - p for p in perm]):
        sketches = edge_sketches(n, [(order[k], order[k + 1]) for k in range(n - 1)])
        scores = [(v * 37) % 101 for v in range(n)]
        index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
        exp = CR.cluster(sketches, CR.JACCARD, 0.1, 0, CR.COMPONENTS, scores)
        top = min(range(n), key=lambda v: (-scores[v], v))
        assert exp == ([0] * n, [top] * n, None, 1)
        try:
            for budget in (1, 3 * n, 0):                    # chunks of 1 query, of 3 queries, the whole index
                pkg.matrix.set_search_many_budget(budget)
                before = count(pkg, "cluster_chunk")
                got = as_lists(index.cluster(0.1, "jaccard", "components", scores=scores))
                assert got == exp, budget
                assert count(pkg, "cluster_chunk") - before == {1: n, 3 * n: -(-n // 3), 0: 1}[budget]
                assert as_lists(index.cluster(0.1, "jaccard", "greedy", scores=scores)) == CR.cluster(sketches, CR.JACCARD, 0.1, 0, CR.GREEDY, scores)
        finally:
            pkg.matrix.set_search_many_budget(0)
        results.append(got)
    assert results[0] == results[1]


# ---------------------------------------------------------------------------------- node tiles

@pytest.mark.parametrize("shape", ["tile-1", "tile", "tile+1", "2tile+1"])
def test_tile_edges(pkg, geometry, shape):
    tile = geometry[1]
    n = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2tile+1": 2 * tile + 1}[shape]
    edges = [(0, n - 1)] + ([(tile - 1, tile)] if n > tile else [])
    sketches = [[10 + v] for v in range(n)]
    for k, (u, v) in enumerate(edges):
        sketches[u].append(5 + k)
        sketches[v].append(5 + k)
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    for linkage in (CR.COMPONENTS, CR.GREEDY):
        cluster, rep, _, k = check(pkg, sketches, CR.JACCARD, 0.2, linkage=linkage, index=index)
        assert k == n - len(edges) and cluster[n - 1] == cluster[0] == 0 and rep[n - 1] == rep[0]
        if n > tile:
            assert cluster[tile] == cluster[tile - 1] and rep[tile] == rep[tile - 1]
        assert sorted(set(cluster)) == list(range(k))


# ---------------------------------------------------------------------------------- the threshold is strict

@pytest.mark.parametrize("metric", [CR.JACCARD, CR.MAX_CONTAINMENT])
def test_threshold_is_strict(pkg, metric):
    # Jaccard 2 / 4 and max-containment 2 / 4: both exactly 0.5
    sketches = {CR.JACCARD: [[1, 2, 3], [2, 3, 4], [9]], CR.MAX_CONTAINMENT: [[1, 2, 3, 4], [3, 4, 5, 6, 7], [9]]}[metric]
    assert CR.SR.value(metric, 2, len(sketches[0]), len(sketches[1])) == 0.5
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    for linkage in (CR.COMPONENTS, CR.GREEDY):
        assert check(pkg, sketches, metric, 0.5, linkage=linkage, index=index)[3] == 3
        assert check(pkg, sketches, metric, math.nextafter(0.5, 0.0), linkage=linkage, index=index)[3] == 2
        assert check(pkg, sketches, metric, 0.0, 3, linkage=linkage, index=index)[3] == 3       # common == 2 < 3
        assert check(pkg, sketches, metric, 0.0, 2, linkage=linkage, index=index)[3] == 2


# ---------------------------------------------------------------------------------- scores

def test_scores(pkg):
    a, b, c = 0, 1, 2
    sketches = edge_sketches(3, [(a, b), (b, c)])
    sketches[b].append(7)                                   # b is the largest: the default order is b, a, c
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    assert check(pkg, sketches, CR.JACCARD, 0.05, linkage=CR.GREEDY, index=index)[:2] == ([0, 0, 0], [b, b, b])
    got = check(pkg, sketches, CR.JACCARD, 0.05, linkage=CR.GREEDY, scores=[3, 1, 2], index=index)
    assert got[:2] == ([0, 0, 1], [a, a, c]) and got[3] == 2
    # equal scores: the lowest node represents
    assert check(pkg, sketches, CR.JACCARD, 0.05, linkage=CR.GREEDY, scores=[4, 4, 4], index=index)[1] == [a, a, c]
    assert check(pkg, sketches, CR.JACCARD, 0.05, scores=[4, 4, 4], index=index)[1] == [a, a, a]
    # the components representative is the top-scored member
    assert check(pkg, sketches, CR.JACCARD, 0.05, index=index)[1] == [b, b, b]
    assert check(pkg, sketches, CR.JACCARD, 0.05, scores=[1, 2, 0xFFFFFFFF], index=index)[1] == [c, c, c]
    assert check(pkg, sketches, CR.JACCARD, 0.05, scores=[0, 0, 0], index=index)[1] == [a, a, a]


# ---------------------------------------------------------------------------------- greedy rounds

def test_greedy_rounds(pkg):
    n = 70
    sketches = edge_sketches(n, [(v, v + 1) for v in range(n - 1)])
    scores = list(range(n, 0, -1))
    adj = CR.graph(sketches, CR.JACCARD, 0.05)
    reps, rounds = CR.greedy_rounds(adj, scores)
    assert rounds == n and reps == set(range(0, n, 2))
    exp = CR.cluster(sketches, CR.JACCARD, 0.05, 0, CR.GREEDY, scores)
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    default = pkg.matrix.cluster_rounds()
    assert default == 32
    try:
        for period in (1, 3, 0):
            pkg.matrix.set_cluster_rounds(period)
            eff = period or default
            assert pkg.matrix.cluster_rounds() == eff
            before = count(pkg, "cluster_round")
            assert as_lists(index.cluster(0.05, "jaccard", "greedy", scores=scores)) == exp, period
            assert count(pkg, "cluster_round") - before == -(-rounds // eff) * eff, period
    finally:
        pkg.matrix.set_cluster_rounds(0)


# ---------------------------------------------------------------------------------- long adjacency lists, and the tie rule

def test_hub(pkg, geometry):
    lane_max, leaves = geometry[0], 3000
    hub = [1000 + k for k in range(leaves)]
    sketches = [hub] + [[h] for h in hub]                   # node 0 is the hub; every leaf is contained in it: value 1.0
    n = leaves + 1
    assert leaves > lane_max >= 1                            # the hub's list is walked by a wave, a leaf's by its lane
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    got = check(pkg, sketches, CR.MAX_CONTAINMENT, 0.5, linkage=CR.GREEDY, index=index)      # the hub is the largest
    assert got == ([0] * n, [0] * n, [leaves] + [1] * leaves, 1)
    assert check(pkg, sketches, CR.MAX_CONTAINMENT, 0.5, index=index)[3] == 1
    # the hub scored lowest: every leaf represents; the hub joins the first in priority, all values being 1.0
    scores = [0] + [1 + (v * 7) % 13 for v in range(1, n)]
    first = min(range(1, n), key=lambda v: (-scores[v], v))
    got = check(pkg, sketches, CR.MAX_CONTAINMENT, 0.5, linkage=CR.GREEDY, scores=scores, index=index)
    assert got[3] == leaves and got[1][0] == first != 1 and got[2][0] == 1 and got[0][0] == got[0][first] == 0
    # on both sides of the lane / wave limit: a hub of lane_max and of lane_max + 1 leaves
    for k in (lane_max, lane_max + 1):
        small = [hub[:k]] + [[h] for h in hub[:k]]
        sc = [0] + [1 + (v * 7) % 5 for v in range(1, k + 1)]
        check(pkg, small, CR.MAX_CONTAINMENT, 0.5, linkage=CR.GREEDY)
        assert check(pkg, small, CR.MAX_CONTAINMENT, 0.5, linkage=CR.GREEDY, scores=sc)[3] == k


# ---------------------------------------------------------------------------------- the pair budget

def raw(pkg, index, n, metric=0, threshold=0.1, linkage=0, rep_common=False, null=None, threshold_common=0):
    """smh_index_cluster on sentinel-filled outputs: (return code, message, the outputs untouched?)"""
    L = pkg.lib()
    u32p = C.POINTER(C.c_uint32)
    arrays = {k: np.full(max(n, 1), SENTINEL, dtype=np.uint32) for k in ("cluster", "representative", "rep_common")}
    k = C.c_uint32(SENTINEL)
    ptr = {name: (a.ctypes.data_as(u32p) if name != null and (name != "rep_common" or rep_common) else None) for name, a in arrays.items()}
    L.sourmash_err_clear()
    rc = L.smh_index_cluster(index._h, metric, threshold, threshold_common, linkage, None, ptr["cluster"], ptr["representative"],
                             ptr["rep_common"], None if null == "n_clusters" else C.byref(k))
    message = ""
    if rc != 0:
        with pytest.raises(pkg.SourmashError) as ei:
            pkg.errors.check()
        assert ei.value.code == rc
        message = ei.value.message
    untouched = all((a == SENTINEL).all() for a in arrays.values()) and k.value == SENTINEL
    return rc, message, untouched


def test_pair_budget(pkg, fx):
    directed = len(fx.index.pairwise(0.0, "jaccard", upper=False))
    assert directed == 2 * 1398
    default = pkg.matrix.cluster_pair_budget()
    assert default == 1 << 27
    try:
        pkg.matrix.set_cluster_pair_budget(directed - 1)
        assert pkg.matrix.cluster_pair_budget() == directed - 1
        rc, message, untouched = raw(pkg, fx.index, 100, linkage=1, threshold=0.0, rep_common=True)
        assert rc == 3 and untouched and str(directed) in message and str(directed - 1) in message
        assert fx.index.cluster(0.0, "jaccard", "components").n_clusters == 2
        pkg.matrix.set_cluster_pair_budget(directed)          # the budget itself is not exceeded
        assert fx.index.cluster(0.0, "jaccard", "greedy").n_clusters == 13
    finally:
        pkg.matrix.set_cluster_pair_budget(0)
    assert pkg.matrix.cluster_pair_budget() == default
    assert fx.index.cluster(0.0, "jaccard", "greedy").n_clusters == 13


# ---------------------------------------------------------------------------------- the other indexes

def test_downsampled_index(pkg, fx):
    scaled = 4 * round(2 ** 64 / fx.max_hash)
    child = fx.index.downsample(scaled=scaled)
    cut_at = child.max_hash
    cut = [[h for h in m if h <= cut_at] for m in fx.mins]
    assert child.sizes().tolist() == [len(c) for c in cut] and sum(map(len, cut)) < sum(fx.sizes)
    rebuilt = pkg.index.ResidentIndex([mk(pkg, c, max_hash=cut_at) for c in cut])
    for metric, linkage in ((CR.JACCARD, CR.COMPONENTS), (CR.MAX_CONTAINMENT, CR.GREEDY)):
        got = as_lists(child.cluster(0.02, NAMES[metric], LINKS[linkage]))
        assert got == as_lists(rebuilt.cluster(0.02, NAMES[metric], LINKS[linkage])) == CR.cluster(cut, metric, 0.02, 0, linkage)
        assert 1 < got[3] < 100
    # threshold_bp goes through the index's scaled
    got = as_lists(child.cluster(0.0, "jaccard", "components", threshold_bp=2.5 * scaled))
    assert got == CR.cluster(cut, CR.JACCARD, 0.0, 3, CR.COMPONENTS)


def test_degenerate_and_ignored_inputs(pkg):
    empty = pkg.index.ResidentIndex([])
    for linkage in ("components", "greedy"):
        res = empty.cluster(0.0, linkage=linkage)
        assert len(res) == 0 and res.n_clusters == 0 and res.sizes().tolist() == []
    for linkage in (CR.COMPONENTS, CR.GREEDY):
        assert check(pkg, [[1, 2, 3]], linkage=linkage)[:2] == ([0], [0])
        assert check(pkg, [[]], linkage=linkage)[3] == 1
        assert check(pkg, [[], []], linkage=linkage)[3] == 2
        got = check(pkg, [[], [1, 2], [], [2, 3], [9], []], linkage=linkage)
        assert got[0] == [0, 1, 2, 1, 3, 4] and got[3] == 5
    # abundances are ignored
    rng = np.random.default_rng(5)
    pool = [int(x) for x in rng.integers(1, M64, 300, dtype=np.uint64)]
    sketches = [[int(x) for x in rng.choice(pool, 40, replace=False)] for _ in range(30)]
    weighted = pkg.index.ResidentIndex([mk(pkg, s, {h: 1 + h % 9 for h in s}) for s in sketches])
    for linkage in (CR.COMPONENTS, CR.GREEDY):
        flat = check(pkg, sketches, CR.JACCARD, 0.12, linkage=linkage)
        assert check(pkg, sketches, CR.JACCARD, 0.12, linkage=linkage, index=weighted) == flat and 1 < flat[3] < 30


def test_ani_threshold(pkg, fx):
    res = fx.index.cluster(0.9, "max_containment", "greedy", ani=True)
    assert as_lists(res) == CR.cluster(fx.mins, CR.MAX_CONTAINMENT, 0.9 ** 21, 0, CR.GREEDY)
    with pytest.raises(ValueError):
        fx.index.cluster(0.9, "jaccard", ani=True)
    prot = pkg.index.ResidentIndex([mk(pkg, [1, 2, 3], protein=True), mk(pkg, [3, 4], protein=True)])
    with pytest.raises(ValueError):
        prot.cluster(0.9, "max_containment", ani=True)
    assert as_lists(prot.cluster(0.3, "max_containment", "greedy")) == ([0, 0], [0, 0], [3, 1], 1)
    with pytest.raises(ValueError):
        fx.index.cluster(0.1, "containment_node")


def test_the_kernels_ran(pkg):
    L = pkg.lib()
    index = pkg.index.ResidentIndex([mk(pkg, [1, 2, 3]), mk(pkg, [3, 4]), mk(pkg, [9])])
    names = ("cluster_probe", "cluster_link", "cluster_finish", "cluster_round", "cluster_assign", "search_many_probe", "search_many_emit")
    L.smh_profile_enable(1)
    try:
        L.smh_profile_reset()
        assert as_lists(index.cluster(0.0)) == ([0, 0, 1], [0, 0, 2], None, 2)
        assert [count(pkg, k) for k in names] == [1, 1, 1, 0, 0, 0, 0]
        assert as_lists(index.cluster(0.0, linkage="greedy")) == ([0, 0, 1], [0, 0, 2], [3, 1, 1], 2)
        assert [count(pkg, k) for k in names] == [1, 1, 2, pkg.matrix.cluster_rounds(), 1, 1, 1]
    finally:
        L.smh_profile_enable(0)


# ---------------------------------------------------------------------------------- errors

def test_errors_write_nothing(pkg):
    nodes = [mk(pkg, [1, 2, 3]), mk(pkg, [3, 4])]
    index = pkg.index.ResidentIndex(nodes)
    assert raw(pkg, index, 2) == (0, "", False)
    for kwargs, code in ((dict(null="cluster"), 1), (dict(null="representative"), 1), (dict(null="n_clusters"), 1),
                         (dict(threshold=float("nan")), 3), (dict(metric=4), 3), (dict(metric=1), 3), (dict(metric=2), 3),
                         (dict(linkage=2), 3), (dict(linkage=0, rep_common=True), 3)):
        rc, message, untouched = raw(pkg, index, 2, **kwargs)
        assert rc == code and untouched, kwargs
    assert "directed" in raw(pkg, index, 2, metric=1)[1] and "rep_common" in raw(pkg, index, 2, rep_common=True)[1]
    mixed = pkg.index.ResidentIndex(nodes + [mk(pkg, [1, 2, 9], num=5)])
    for linkage in (0, 1):
        rc, message, untouched = raw(pkg, mixed, 3, linkage=linkage)
        assert rc == 3 and "num sketch" in message and untouched
        rc, message, untouched = raw(pkg, pkg.index.ResidentIndex(nodes + [mk(pkg, [5], seed=43)]), 3, linkage=linkage)
        assert rc == 104 and untouched                       # nodes that refuse each other: as search_self
    assert raw(pkg, index, 2, linkage=1, rep_common=True) == (0, "", False), "a refusal leaves the index usable"
