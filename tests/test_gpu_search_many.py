"""The thresholded search of a batch on the device (smh_index_search_many, smh_index_search_block_dev, smh_index_search_self;
ResidentIndex.search_many / search_block_dev / pairwise) against the plain-Python restatement: the rows must be EQUAL -- every
output is an integer.  ResidentIndex.find per query (the nodes) and ResidentIndex.compare(want=("count_common",)) (the counts)
are the second witnesses.  The shapes stand on both sides of the sizes smh_search_geometry and smh_match_geometry report."""
import ctypes as C
import math

import numpy as np
import pytest

import search_many_restatement as SR

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
SENTINEL = 0xDEADBEEFDEADBEEF
NAMES = {SR.JACCARD: "jaccard", SR.CONTAINMENT_NODE: "containment_node", SR.CONTAINMENT_QUERY: "containment_query",
         SR.MAX_CONTAINMENT: "max_containment"}


def mk(pkg, hashes, abunds=None, max_hash=M64, ksize=21, seed=42, protein=False, num=0):
    """a sketch holding `hashes`; abunds ({hash: abundance}) makes it track abundances"""
    mh = pkg.KmerMinHash(num, ksize, protein, seed, max_hash, abunds is not None)
    h = sorted(int(x) for x in hashes)
    if abunds is not None and h:
        mh.add_many_with_abund([(x, abunds[x]) for x in h])
    elif h:
        mh.add_many(np.array(h, dtype=np.uint64))
    return mh


def per_query(res):
    """a SearchResult as the restatement writes it: per query the tuples (node, common, node_size, query_size)"""
    rows = list(zip(res.node.tolist(), res.common.tolist(), res.node_size.tolist(), res.query_size.tolist()))
    off = [int(x) for x in res.offsets]
    assert off[0] == 0 and off[-1] == len(rows) and off == sorted(off)
    return [rows[a:b] for a, b in zip(off, off[1:])]


def run(index, queries, metric, threshold, threshold_common=0):
    return per_query(index.search_many(queries, threshold, NAMES[metric], threshold_bp=threshold_common, scaled=1))


def check(pkg, sketches, queries, metric=SR.JACCARD, threshold=0.0, threshold_common=0, index=None):
    index = index or pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    got = run(index, [mk(pkg, q) for q in queries], metric, threshold, threshold_common)
    assert got == SR.search_many(sketches, queries, metric, threshold, threshold_common)
    return got


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


@pytest.fixture(scope="module")
def geometry(pkg):
    short_owners, tile, max_queries = pkg.matrix.search_geometry()
    assert 2 <= short_owners < 62 and tile >= 128 and max_queries == SR.MAX_QUERIES
    return short_owners, tile, max_queries


# ---------------------------------------------------------------------------------- the committed fixture

class Fixture:
    def __init__(self, pkg, sketches):
        self.mins = [s["mins"] for s in sketches]
        self.max_hash = sketches[0]["max_hash"]
        self.abs = [dict(zip(s["mins"], s["abundances"])) for s in sketches]
        unions = [sorted(set().union(*(self.mins[i] for i in pick))) for pick in ((0, 1), (5, 40, 77), range(0, 100, 9), range(100))]
        everything = set(unions[-1])
        foreign = [h + 1 for h in unions[-1][:300] if h + 1 not in everything]
        self.q_hashes = self.mins + unions + [foreign]
        self.index = pkg.index.ResidentIndex([mk(pkg, m, ab, max_hash=self.max_hash) for m, ab in zip(self.mins, self.abs)])
        self.queries = [mk(pkg, q, max_hash=self.max_hash) for q in self.q_hashes]
        self.shared = SR.shared(self.mins, self.q_hashes)      # once: every metric and threshold selects among these


@pytest.fixture(scope="module")
def fx(pkg, sbt_subset_sketches):
    return Fixture(pkg, sbt_subset_sketches)


@pytest.mark.parametrize("metric", SR.METRICS)
def test_fixture_batch(fx, metric):
    reported = []
    for threshold in (0.0, 0.1, 1.0):                        # 1.0: above every value
        got = per_query(fx.index.search_many(fx.queries, threshold, NAMES[metric]))
        exp = SR.select(fx.shared, metric, threshold)
        assert got == exp, threshold
        reported.append(sum(map(len, got)))
        if metric in (SR.JACCARD, SR.CONTAINMENT_NODE):      # the nodes, and their order, are find's
            for q, rows in enumerate(got):
                assert [r[0] for r in rows] == fx.index.find(fx.queries[q], threshold, containment=metric == SR.CONTAINMENT_NODE), (threshold, q)
    assert reported[0] > reported[1] > reported[2] == 0 and reported[0] > 300
    assert got[-1] == [] and exp[-1] == []                   # the foreign query


def test_fixture_counts_are_compare_s(pkg, fx):
    cc = fx.index.compare(pkg.index.ResidentIndex(fx.queries), want=("count_common",))["count_common"]
    res = fx.index.search_many(fx.queries, 0.0, "containment_query")
    got = np.zeros_like(cc)
    got[res.node, res.query()] = res.common
    assert np.array_equal(got, cc) and len(res) == int((cc > 0).sum())
    # the floats derived on the host are the restatement's values, and ANI is theirs to the 1 / ksize
    rows = [r for q in per_query(res) for r in q]
    for name, metric in (("jaccard", SR.JACCARD), ("containment_node", SR.CONTAINMENT_NODE), ("containment_query", SR.CONTAINMENT_QUERY),
                         ("max_containment", SR.MAX_CONTAINMENT)):
        assert getattr(res, name).tolist() == [SR.value(metric, c, lq, ls) for _, c, ls, lq in rows]
    # (numpy's pow and Python's may differ in the last place: both are libm-grade, neither is the rule)
    assert res.ksize == 21 and res.ani().tolist() == pytest.approx([SR.value(SR.CONTAINMENT_QUERY, c, lq, ls) ** (1.0 / 21) for _, c, ls, lq in rows], rel=1e-14)


def test_threshold_bp_goes_through_scaled(fx):
    scaled = round(2 ** 64 / fx.max_hash)
    got = per_query(fx.index.search_many(fx.queries[:20], 0.0, "jaccard", threshold_bp=9.5 * scaled))
    assert got == SR.select(fx.shared[:20], SR.JACCARD, 0.0, 10) and 0 < sum(map(len, got)) < sum(map(len, fx.shared[:20]))


# ---------------------------------------------------------------------------------- the threshold itself

@pytest.mark.parametrize("metric", SR.METRICS)
def test_exact_threshold(pkg, metric):
    """pairs whose value IS the threshold (out: the comparison is strict), and the doubles next to it on both sides"""
    # (common, node_size, query_size); the nodes and queries are disjoint but for their `common` hashes
    shapes = [(1, 2, 1), (1, 3, 3), (2, 7, 5), (3, 10, 9), (7, 11, 13), (5, 5, 5), (1, 49, 7)]
    sketches, queries, base = [], [], 1000
    for c, ls, lq in shapes:
        sketches.append(list(range(base, base + ls)))
        queries.append(list(range(base + ls - c, base + ls - c + lq)))
        base += 1000
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    qs = [mk(pkg, q) for q in queries]
    for k, (c, ls, lq) in enumerate(shapes):
        v = SR.value(metric, c, lq, ls)
        for threshold, inside in ((v, False), (math.nextafter(v, 0.0), True), (math.nextafter(v, 2.0), False)):
            got = run(index, qs, metric, threshold)
            assert got == SR.search_many(sketches, queries, metric, threshold)
            assert (got[k] == [(k, c, ls, lq)]) == inside and (got[k] == []) != inside, (k, threshold)


# ---------------------------------------------------------------------------------- owner lists

def test_owner_list_edges(pkg, geometry):
    """hashes held by short - 1, short, short + 1, 63, 64, 65 and 3 000 nodes: lists walked by a lane and by the wave"""
    short, n = geometry[0], 3000
    lengths = (short - 1, short, short + 1, 63, 64, 65, n)
    held = {k: (1 << 60) + k for k in lengths}
    sketches = [[h for k, h in held.items() if i < k] + [100 + i] for i in range(n)]
    queries = [[h] for h in held.values()] + [sorted(held.values()), sorted(held.values()) + [100, 100 + n - 1, 99]]
    got = check(pkg, sketches, queries, SR.CONTAINMENT_QUERY, 0.0)
    assert [len(g) for g in got] == list(lengths) + [n, n]
    assert got[-1][0] == (0, len(lengths) + 1, len(lengths) + 1, len(lengths) + 3) and got[-1][-1] == (n - 1, 2, 2, len(lengths) + 3)
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches[:70]])
    assert check(pkg, sketches[:70], queries, SR.JACCARD, 0.2, index=index)[-2][0][1] == len(lengths)


# ---------------------------------------------------------------------------------- node tiles

@pytest.mark.parametrize("shape", ["tile-1", "tile", "tile+1", "2tile+1"])
def test_node_tile_edges(pkg, geometry, shape):
    tile = geometry[1]
    n = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2tile+1": 2 * tile + 1}[shape]
    sketches = [[10 + i] for i in range(n)]                  # node i alone holds 10 + i
    # survivors at the first and the last node of a tile, at the edges of a wave's 64 nodes; the second tile of 2 tile + 1 has none
    at = sorted({i for i in (0, 1, 63, 64, 65, 255, 256, tile - 2, tile - 1, tile, n - 1) if 0 <= i < n and not tile < i < 2 * tile})
    queries = [[10 + i for i in at], [10 + i for i in range(n)], [10 + n - 1], [10], [9]]
    got = check(pkg, sketches, queries, SR.CONTAINMENT_NODE, 0.5)
    assert [r[0] for r in got[0]] == at and [r[0] for r in got[1]] == list(range(n)) and got[4] == []
    if shape == "2tile+1":
        assert not [r for r in got[0] if tile < r[0] < 2 * tile] and got[0][-1][0] == 2 * tile
    # the self mode over the same tiles: everybody also holds one hash, so every pair survives
    nodes = [mk(pkg, s + [5]) for s in sketches]
    index = pkg.index.ResidentIndex(nodes)
    for upper in (True, False):
        res = index.pairwise(0.0, "jaccard", upper=upper)
        off = res.offsets.astype(np.int64)
        assert np.array_equal(np.diff(off), [n - 1 - q if upper else n - 1 for q in range(n)])
        for q in (0, 1, tile - 2, n - 2, n - 1):
            want = [i for i in range(n) if (i > q if upper else i != q)]
            assert res.node[off[q]:off[q + 1]].tolist() == want
        assert (res.common == 1).all() and (res.node_size == 2).all() and (res.query_size == 2).all()


# ---------------------------------------------------------------------------------- the directory search

@pytest.mark.parametrize("delta", [-1, 0, 1, "x4"])
def test_directory_search_edges(pkg, delta):
    P = pkg.matrix.match_geometry()[2]
    size = 4 * P + 3 if delta == "x4" else P + delta
    U = [1000 + 10 * i for i in range(size)]
    sketches = [U[::2], U[1::2], sorted(set(U[::7] + [U[-1]])), U[: size // 2]]
    shift = 0
    while -(-size // (1 << shift)) > P:
        shift += 1
    step = 1 << shift
    at = sorted({i for s in range(0, size, max(step, size // 40 // step * step)) for i in (s - 1, s, s + 1) if 0 <= i < size}
                | {0, 1, size - 2, size - 1, (size - 1) // step * step})
    queries = [[U[0], U[-1]],
               [U[i] for i in at],
               [U[0] - 1, 5, U[-1] + 1, M64, U[3] + 1, U[size // 2] + 5],          # below, above, between: nothing held
               [U[0] - 1, U[0], U[1] + 1, U[-1], U[-1] + 1] + [U[i] + 3 for i in at],
               U[::3]]
    got = check(pkg, sketches, queries, SR.CONTAINMENT_QUERY, 0.0)
    assert sum(r[1] for r in got[0]) >= 3 and got[2] == [] and sum(r[1] for r in got[3]) >= 3   # both ends were found
    assert sum(r[1] for r in got[1] if r[0] < 2) == len(at)                                    # every probed rank was found


# ---------------------------------------------------------------------------------- queries

def test_query_edges(pkg):
    sketches = [[1, 2, 3], [3, 4], [], [7, 8, 9, 10]]
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    a, b = [1, 2, 3, 4], [8, 9, 11]
    for queries in ([[], a, b], [a, b, []], [a, [], [], b], [[], [], a, [], b, []], [a, a], [a, b, a, b], [[]], [[], []]):
        for metric in SR.METRICS:
            got = check(pkg, sketches, queries, metric, 0.3, index=index)
            for q, rows in zip(queries, got):
                assert rows == got[queries.index(q)]          # the same sketch gives the same rows
    res = index.search_many([], 0.0)
    assert len(res) == 0 and res.offsets.tolist() == [0]
    empty = pkg.index.ResidentIndex([])
    assert run(empty, [mk(pkg, a), mk(pkg, [])], SR.JACCARD, 0.0) == [[], []]
    assert len(empty.pairwise(0.0)) == 0 and empty.pairwise(0.0).offsets.tolist() == [0]
    hollow = pkg.index.ResidentIndex([mk(pkg, []), mk(pkg, [])])
    assert run(hollow, [mk(pkg, a)], SR.CONTAINMENT_NODE, 0.0) == [[]] and per_query(hollow.pairwise(0.0, upper=False)) == [[], []]
    assert run(index, [mk(pkg, [20, 21])], SR.JACCARD, -1.0) == [[]], "a pair that shares nothing is never reported"


def test_abundances_do_not_matter(pkg):
    rng = np.random.default_rng(3)
    pool = [int(x) for x in rng.integers(1, M64, 400, dtype=np.uint64)]
    sketches = [[int(x) for x in rng.choice(pool, 60, replace=False)] for _ in range(20)]
    queries = [[int(x) for x in rng.choice(pool, k, replace=False)] for k in (5, 90, 400)]
    flat = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    weighted = pkg.index.ResidentIndex([mk(pkg, s, {h: 1 + h % 9 for h in s}) for s in sketches])
    q_flat = [mk(pkg, q) for q in queries]
    q_weighted = [mk(pkg, q, {h: 2 + h % 5 for h in q}) for q in queries]
    exp = SR.search_many(sketches, queries, SR.MAX_CONTAINMENT, 0.05)
    for index in (flat, weighted):
        for qs in (q_flat, q_weighted, [q_flat[0], q_weighted[1], q_flat[2]]):
            assert run(index, qs, SR.MAX_CONTAINMENT, 0.05) == exp
    assert sum(map(len, exp)) > 20


# ---------------------------------------------------------------------------------- chunks

def test_chunking_changes_no_result(pkg):
    rng = np.random.default_rng(14)
    n, nq = 50, 9
    universe = [int(x) for x in rng.integers(0, M64, 2000, dtype=np.uint64)]
    sketches = [[int(x) for x in rng.choice(universe, 120, replace=False)] for _ in range(n)]
    queries = [[int(x) for x in rng.choice(universe, (100 + 50 * k) * (k != 4), replace=False)] for k in range(nq)]   # (one is empty)
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    L = pkg.lib()
    default = pkg.matrix.search_many_budget()
    assert default == 1 << 26
    base = check(pkg, sketches, queries, SR.JACCARD, 0.02, index=index)
    assert sum(map(len, base)) > 100 and min(map(len, base)) == 0
    own = per_query(index.pairwise(0.02, upper=False))
    qs = [mk(pkg, q) for q in queries]
    sizes = [len(q) for q in queries]
    try:
        for budget in (n - 1, n, 2 * n, 2 * n + 1, 0):
            pkg.matrix.set_search_many_budget(budget)
            eff = budget or default
            assert pkg.matrix.search_many_budget() == eff
            # twice: the first call of a shape creates the blocks the pool has never seen, the second takes them and
            # must give every one of them back
            for again in (False, True):
                pool = L.smh_pool_bytes()
                before = count(pkg, "search_many_chunk")
                assert run(index, qs, SR.JACCARD, 0.02) == base, budget
                assert count(pkg, "search_many_chunk") - before == len(SR.cut_chunks(sizes, n, eff)), budget
                before = count(pkg, "search_many_chunk")
                assert per_query(index.pairwise(0.02, upper=False)) == own, budget
                assert count(pkg, "search_many_chunk") - before == len(SR.cut_chunks([120] * n, n, eff)), budget
                assert not again or L.smh_pool_bytes() == pool, budget
    finally:
        pkg.matrix.set_search_many_budget(0)
    assert [len(SR.cut_chunks([1] * nq, n, b)) for b in (n - 1, n, 2 * n, 2 * n + 1, default)] == [9, 9, 5, 5, 1]


def csr_on_device(pkg, hashes_per_query):
    import torch
    flat, off = pkg.matrix.csr_from_sketches([np.array(sorted(q), dtype=np.uint64) for q in hashes_per_query])
    t = torch.from_numpy(flat.view(np.int64)).cuda() if flat.size else torch.zeros(1, dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    return t, off


def test_one_grid_dimension_of_queries(pkg, geometry):
    """(largest queries per chunk) + 1 tiny queries through the CSR form: two chunks, the second of one query"""
    nq = geometry[2] + 1
    sketches = [[1, 2], [2, 3, 4]]
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    kinds = [[1], [2], [3, 4], [], [5], [1, 2, 3, 4]]
    rng = np.random.default_rng(1)
    pick = rng.integers(0, len(kinds), nq)
    pick[-1] = 1                                            # the query that is alone in the second chunk hits both nodes
    import torch
    lens = np.array([len(kinds[k]) for k in pick], dtype=np.uint64)
    off = np.zeros(nq + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    flat = np.array([h for k in pick for h in kinds[k]], dtype=np.uint64)
    t = torch.from_numpy(flat.view(np.int64)).cuda()
    torch.cuda.synchronize()
    before = count(pkg, "search_many_chunk")
    res = index.search_block_dev(t.data_ptr(), off, 0.0, "jaccard")
    assert count(pkg, "search_many_chunk") - before == 2
    by_kind = SR.search_many(sketches, kinds, SR.JACCARD, 0.0)
    exp_counts = np.array([len(by_kind[k]) for k in pick])
    assert np.array_equal(np.diff(res.offsets.astype(np.int64)), exp_counts)
    exp_rows = np.array([r for k in pick for r in by_kind[k]], dtype=np.uint32)
    got_rows = np.stack([res.node, res.common, res.node_size, res.query_size], axis=1)
    assert np.array_equal(got_rows, exp_rows) and per_query(res)[-1] == [(0, 1, 2, 1), (1, 1, 3, 1)]


# ---------------------------------------------------------------------------------- the other forms

def test_csr_device_form(pkg, fx):
    t, off = csr_on_device(pkg, fx.q_hashes)
    for metric, threshold, thc in ((SR.JACCARD, 0.1, 0), (SR.MAX_CONTAINMENT, 0.0, 25)):
        res = fx.index.search_block_dev(t.data_ptr(), off, threshold, NAMES[metric], threshold_common=thc)
        assert per_query(res) == run(fx.index, fx.queries, metric, threshold, thc) == SR.select(fx.shared, metric, threshold, thc)
    # an offset that is not 0: the batch is its tail
    res = fx.index.search_block_dev(t.data_ptr(), off[90:], 0.1, "jaccard")
    assert per_query(res) == SR.select(fx.shared[90:], SR.JACCARD, 0.1)
    # a CSR carries no parameters: an index that does not speak with one voice is refused, and nothing is written
    odd = pkg.index.ResidentIndex([mk(pkg, fx.mins[0], max_hash=fx.max_hash), mk(pkg, fx.mins[1], max_hash=fx.max_hash, seed=43)])
    with pytest.raises(pkg.SourmashError) as ei:
        odd.search_block_dev(t.data_ptr(), off, 0.1)
    assert ei.value.code == 3 and "same ksize" in ei.value.message


def test_queries_resident_on_the_device(pkg, pyoracle):
    mx = M64 // 20
    genome = pyoracle.synth_dna(0, 30000, 21)
    parts = [genome[a:b] for a, b in ((0, 12000), (8000, 20000), (15000, 30000), (0, 30000))]

    def sketched(part, track):
        mh = pkg.KmerMinHash(0, 21, False, 42, mx, track)
        mh.add_sequence(part, True)
        return mh

    nodes = [sketched(genome[a:a + 4000], False) for a in range(0, 30000, 3000)]
    node_mins = [m.mins for m in nodes]
    index = pkg.index.ResidentIndex(nodes)
    for track in (True, False):
        hosts = [mk(pkg, t.mins, max_hash=mx) for t in [sketched(p, track) for p in parts]]
        resident = [sketched(p, track) for p in parts]
        batch = [resident[0], hosts[1], resident[2], resident[3]]          # HBM and host states in one batch
        before = count(pkg, "sketch_to_host")
        got = run(index, batch, SR.CONTAINMENT_NODE, 0.2)
        assert count(pkg, "sketch_to_host") == before, "search_many brought a device-resident query to the host"
        assert got == run(index, hosts, SR.CONTAINMENT_NODE, 0.2) == SR.search_many(node_mins, [h.mins for h in hosts], SR.CONTAINMENT_NODE, 0.2)
        assert len(got[3]) == 10 and 3 <= len(got[0]) < len(got[3])
        assert resident[0].mins == hosts[0].mins              # they were resident: looking at one moves it now
        assert count(pkg, "sketch_to_host") == before + 1


# ---------------------------------------------------------------------------------- the index against itself

@pytest.mark.parametrize("metric", SR.METRICS)
def test_pairwise_is_search_many_filtered(pkg, fx, metric):
    full = run(fx.index, fx.queries[:100], metric, 0.05)
    assert full == SR.select(fx.shared[:100], metric, 0.05)
    for upper in (True, False):
        got = per_query(fx.index.pairwise(0.05, NAMES[metric], upper=upper))
        assert got == [[r for r in rows if (r[0] > q if upper else r[0] != q)] for q, rows in enumerate(full)]
        assert got == SR.search_self(fx.mins, metric, 0.05, upper_only=upper) and sum(map(len, got)) > 50


def test_pairwise_of_a_downsampled_index(pkg, fx):
    """the nodes of index.downsample() are the uncut sketches: pairwise reads the cut ones where they lie"""
    cut_at = fx.max_hash // 4
    child = fx.index.downsample(max_hash=cut_at)
    assert len(child.nodes[0]) == len(fx.mins[0]), "the Python nodes of a downsampled index are the uncut sketches"
    cut = [[h for h in m if h <= cut_at] for m in fx.mins]
    rebuilt = pkg.index.ResidentIndex([mk(pkg, m, max_hash=fx.max_hash).downsample_max_hash(cut_at) for m in fx.mins])
    for metric, thr_bp in ((SR.JACCARD, 0), (SR.CONTAINMENT_QUERY, 3 * round(2 ** 64 / cut_at))):
        for upper in (True, False):
            got = per_query(child.pairwise(0.02, NAMES[metric], threshold_bp=thr_bp, upper=upper))
            assert got == per_query(rebuilt.pairwise(0.02, NAMES[metric], threshold_bp=thr_bp, upper=upper))
            assert got == SR.search_self(cut, metric, 0.02, 3 if thr_bp else 0, upper_only=upper) and sum(map(len, got)) > 20
    # and the batch form meets the queries at the index's resolution
    many = per_query(fx.index.search_many([mk(pkg, m, max_hash=cut_at) for m in cut[:7]] + fx.queries[7:12], 0.02, downsample=True))
    assert many[:7] == SR.search_many(cut, cut[:7], SR.JACCARD, 0.02) and many[7:] == SR.select(fx.shared[7:12], SR.JACCARD, 0.02)


# ---------------------------------------------------------------------------------- one directory for everybody

def test_shared_directory(pkg, pyoracle):
    genome = pyoracle.synth_dna(0, 3000, 4)
    records = [genome[:200], genome[200:500]]
    probe = pkg.KmerMinHash(0, 21, False, 42, M64, False)
    probe.add_sequence(genome[:1000], True)
    ws = probe.mins
    sketches = [ws[::2], ws[1::2], ws[::5]]
    queries = [ws[::3], ws[:300]]
    qs = [mk(pkg, q) for q in queries]
    exp = SR.search_many(sketches, queries, SR.JACCARD, 0.0)

    def fresh():
        return pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])

    built = count(pkg, "match_directory_built")
    first = fresh()
    assert run(first, qs, SR.JACCARD, 0.0) == exp                 # search builds it ...
    assert count(pkg, "match_directory_built") == built + 1
    first.match(records); first.gather_many(qs); first.pairwise(0.0)
    assert count(pkg, "match_directory_built") == built + 1       # ... and match and gather_many find it there
    for opener in (lambda ix: ix.match(records), lambda ix: ix.gather_many(qs)):
        other = fresh()
        opener(other)
        now = count(pkg, "match_directory_built")
        assert run(other, qs, SR.JACCARD, 0.0) == exp and per_query(other.pairwise(0.0)) == SR.search_self(sketches, SR.JACCARD, 0.0, upper_only=True)
        assert count(pkg, "match_directory_built") == now
    assert count(pkg, "match_directory_built") == built + 3


def test_the_kernels_ran(pkg):
    L = pkg.lib()
    index = pkg.index.ResidentIndex([mk(pkg, [1, 2, 3]), mk(pkg, [3, 4])])
    qs = [mk(pkg, [1, 2, 3, 4]), mk(pkg, [4])]
    L.smh_profile_enable(1)
    try:
        L.smh_profile_reset()
        assert run(index, qs, SR.JACCARD, 0.0) == [[(0, 3, 3, 4), (1, 2, 2, 4)], [(1, 1, 2, 1)]]
        assert [count(pkg, k) for k in ("search_many_probe", "search_many_select", "search_many_emit")] == [1, 1, 1]
        assert per_query(index.pairwise(0.0)) == [[(1, 1, 2, 3)], []]
        assert [count(pkg, k) for k in ("search_many_probe", "search_many_select", "search_many_emit")] == [2, 2, 2]
        assert run(index, qs, SR.JACCARD, 1.0) == [[], []]        # nothing survives: no rows are emitted
        assert [count(pkg, k) for k in ("search_many_probe", "search_many_select", "search_many_emit")] == [3, 3, 2]
        assert count(pkg, "compare_wave") + count(pkg, "compare_few") + count(pkg, "compare_pair") + count(pkg, "compare_tiled") == 0, \
            "the batch went through the compare route"
    finally:
        L.smh_profile_enable(0)


# ---------------------------------------------------------------------------------- errors

def test_errors_write_nothing(pkg):
    L = pkg.lib()
    u64p = C.POINTER(C.c_uint64)
    nodes = [mk(pkg, [1, 2, 3]), mk(pkg, [3, 4])]
    index = pkg.index.ResidentIndex(nodes)
    good = [mk(pkg, [1, 2, 3, 4]) for _ in range(5)]
    assert [len(r) for r in run(index, good, SR.JACCARD, 0.0)] == [2] * 5

    def raw(idx, queries, metric=0, threshold=0.1, null_rows=False, null_offsets=False):
        arr = (C.c_void_p * len(queries))(*[q._p for q in queries])
        row_off = np.full(len(queries) + 1, SENTINEL, dtype=np.uint64)
        rows_p = C.POINTER(pkg._lib.SmhSearchRow)()
        L.sourmash_err_clear()
        rc = L.smh_index_search_many(idx._h, arr, len(queries), metric, threshold, 0, None if null_offsets else row_off.ctypes.data_as(u64p),
                                     None if null_rows else C.byref(rows_p))
        assert rc != 0 and not rows_p and (row_off == SENTINEL).all()
        with pytest.raises(pkg.SourmashError) as ei:
            pkg.errors.check()
        assert ei.value.code == rc
        return ei.value

    e = raw(index, good[:3] + [mk(pkg, [1, 2], num=5)] + good[4:])
    assert e.code == 3 and "query 3" in e.message and "scaled" in e.message
    e = raw(index, [good[0], mk(pkg, [1, 2], ksize=31), good[2], mk(pkg, [1, 2], num=5), mk(pkg, [1, 2], seed=43)])
    assert e.code == 101 and "query 1" in e.message              # the lowest failing query, whatever the later ones are
    e = raw(index, [good[0], good[1], mk(pkg, [1, 2], seed=43), mk(pkg, [1, 2], ksize=31)])
    assert e.code == 104 and "query 2" in e.message
    e = raw(index, [mk(pkg, [1, 2], protein=True)] + good)
    assert e.code == 102 and "query 0" in e.message
    mixed = pkg.index.ResidentIndex(nodes + [mk(pkg, [1, 2, 9], num=5)])
    e = raw(mixed, good)
    assert e.code == 3 and "query 0" in e.message and "num sketch" in e.message
    assert raw(index, good, threshold=float("nan")).code == 3 and raw(index, good, metric=4).code == 3
    assert raw(index, good, null_rows=True).code == 1 and raw(index, good, null_offsets=True).code == 1
    with pytest.raises(pkg.SourmashError) as ei:
        index.search_many(good[:2] + [mk(pkg, [1], max_hash=1 << 62)], 0.1, scaled=1)
    assert ei.value.code == 103 and "query 2" in ei.value.message
    for call in (lambda: mixed.pairwise(0.1), lambda: index.pairwise(float("nan")),
                 lambda: pkg.index.ResidentIndex(nodes + [mk(pkg, [5], seed=43)]).pairwise(0.1)):
        with pytest.raises(pkg.SourmashError) as ei:
            call()
        assert ei.value.code in (3, 104)
    assert [len(r) for r in run(index, good, SR.JACCARD, 0.0)] == [2] * 5, "a refusal leaves the index usable"
    # protein indexes are searched like any other; ANI is not guessed for them
    prot = pkg.index.ResidentIndex([mk(pkg, [1, 2, 3], protein=True), mk(pkg, [3, 4], protein=True)])
    res = prot.search_many([mk(pkg, [1, 2, 3, 4], protein=True)], 0.0, "containment_query")
    assert per_query(res) == [[(0, 3, 3, 4), (1, 2, 2, 4)]] and res.containment_query.tolist() == [0.75, 0.5]
    with pytest.raises(ValueError):
        res.ani()
