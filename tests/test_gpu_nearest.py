"""The nearest neighbours of a batch on the device (smh_index_nearest_many, smh_index_nearest_block_dev, smh_index_nearest_self;
ResidentIndex.nearest / nearest_block_dev / knn) against the plain-Python restatement: the rows must be EQUAL, in order -- every
output is an integer.  search_many + np.lexsort + truncation and most_common are the second and third witnesses.  The shapes
stand on both sides of the sizes smh_nearest_geometry and smh_search_geometry report."""
import ctypes as C
import gc

import numpy as np
import pytest

import nearest_restatement as NR
import search_many_restatement as SR

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
SENTINEL = 0xDEADBEEFDEADBEEF
NAMES = {SR.JACCARD: "jaccard", SR.CONTAINMENT_NODE: "containment_node", SR.CONTAINMENT_QUERY: "containment_query",
         SR.MAX_CONTAINMENT: "max_containment"}
TEST_BYTE = 0x5A               # a pattern that is no valid count, offset, node or value


def mk(pkg, hashes, max_hash=M64, ksize=21, seed=42, protein=False, num=0):
    mh = pkg.KmerMinHash(num, ksize, protein, seed, max_hash, False)
    h = sorted(int(x) for x in hashes)
    if h:
        mh.add_many(np.array(h, dtype=np.uint64))
    return mh


def build(pkg, sketches):
    return pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])


def per_query(res):
    """a SearchResult as the restatement writes it: per query the tuples (node, common, node_size, query_size), in order"""
    rows = list(zip(res.node.tolist(), res.common.tolist(), res.node_size.tolist(), res.query_size.tolist()))
    off = [int(x) for x in res.offsets]
    assert off[0] == 0 and off[-1] == len(rows) and off == sorted(off)
    return [rows[a:b] for a, b in zip(off, off[1:])]


def run(index, queries, k, metric, threshold=0.0, threshold_common=0):
    return per_query(index.nearest(queries, k, NAMES[metric], threshold, threshold_bp=threshold_common, scaled=1))


def check(pkg, sketches, queries, k, metric=SR.JACCARD, threshold=0.0, threshold_common=0, index=None, qs=None):
    index = index or build(pkg, sketches)
    got = run(index, qs or [mk(pkg, q) for q in queries], k, metric, threshold, threshold_common)
    assert got == NR.nearest(sketches, queries, k, metric, threshold, threshold_common), (k, metric, threshold)
    return got


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


@pytest.fixture(scope="module")
def geometry(pkg):
    max_k, tile, slots = pkg.matrix.nearest_geometry()
    assert tile == pkg.matrix.search_geometry()[1] and 100 <= max_k < slots and tile <= slots and max_k == NR.MAX_K
    return max_k, tile, slots


# ---------------------------------------------------------------------------------- the committed fixture

class Fixture:
    """the batch of test_gpu_search_many.py, built again here: the 100 fixture sketches as nodes; as queries each of them, four
    unions of them and one query of hashes nobody holds"""

    def __init__(self, pkg, sketches):
        self.mins = [s["mins"] for s in sketches]
        self.max_hash = sketches[0]["max_hash"]
        unions = [sorted(set().union(*(self.mins[i] for i in pick))) for pick in ((0, 1), (5, 40, 77), range(0, 100, 9), range(100))]
        everything = set(unions[-1])
        foreign = [h + 1 for h in unions[-1][:300] if h + 1 not in everything]
        self.q_hashes = self.mins + unions + [foreign]
        self.index = pkg.index.ResidentIndex([mk(pkg, m, max_hash=self.max_hash) for m in self.mins])
        self.queries = [mk(pkg, q, max_hash=self.max_hash) for q in self.q_hashes]
        self.shared = SR.shared(self.mins, self.q_hashes)      # once: every metric, threshold and k selects among these
        self._exp = {}

    def expected(self, k, metric, threshold):
        key = (k, metric, threshold)
        if key not in self._exp:
            self._exp[key] = NR.select(self.shared, k, metric, threshold)
        return self._exp[key]


@pytest.fixture(scope="module")
def fx(pkg, sbt_subset_sketches):
    return Fixture(pkg, sbt_subset_sketches)


@pytest.mark.parametrize("metric", SR.METRICS)
def test_fixture_batch(fx, geometry, metric):
    sizes = []
    for threshold in (0.0, 0.1):
        for k in (1, 3, 100, geometry[0]):
            got = per_query(fx.index.nearest(fx.queries, k, NAMES[metric], threshold))
            assert got == fx.expected(k, metric, threshold), (k, threshold)
            sizes.append(sum(map(len, got)))
            assert got[-1] == []                               # the foreign query
    assert sizes[0] < sizes[1] < sizes[2] <= sizes[3] and sizes[4] < sizes[5] <= sizes[6] < sizes[2]
    assert max(map(len, fx.expected(3, metric, 0.1))) == 3, "k cuts some query of the fixture under both thresholds"


@pytest.mark.parametrize("metric", SR.METRICS)
def test_second_witness_search_many_sorted_on_the_host(fx, metric):
    """search_many + np.lexsort by (value descending, node) + truncation: the route a caller had to take before"""
    full = fx.index.search_many(fx.queries, 0.0, NAMES[metric])
    value = getattr(full, NAMES[metric])
    off = full.offsets.astype(np.int64)
    for k in (3, 100):
        res = fx.index.nearest(fx.queries, k, NAMES[metric])
        want_off, picks = [0], []
        for q in range(len(fx.queries)):
            sl = slice(off[q], off[q + 1])
            order = np.lexsort((full.node[sl], -value[sl]))[:k] + off[q]
            picks.append(order)
            want_off.append(want_off[-1] + len(order))
        pick = np.concatenate(picks)
        assert res.offsets.tolist() == want_off
        for name in ("node", "common", "node_size", "query_size"):
            assert np.array_equal(getattr(res, name), getattr(full, name)[pick]), (name, k)
        assert np.array_equal(getattr(res, NAMES[metric]), value[pick])
        v = getattr(res, NAMES[metric])
        for q in range(len(fx.queries)):
            assert (np.diff(v[res.rows_of(q)]) <= 0).all()


def test_third_witness_most_common(fx):
    res = fx.index.nearest(fx.queries, 1, "containment_query")
    named = 0
    for q, rows in enumerate(per_query(res)):
        if fx.shared[q]:
            node, common = fx.index.most_common(fx.queries[q])
            assert [(r[0], r[1]) for r in rows] == [(node, common)], q
            named += 1
        else:
            assert rows == []
    assert named == len(fx.queries) - 1
    assert res.ksize == 21 and len(res.ani()) == named         # a SearchResult like any other


# ---------------------------------------------------------------------------------- ties

@pytest.mark.parametrize("metric", [SR.CONTAINMENT_NODE, SR.JACCARD, SR.MAX_CONTAINMENT])
def test_ties_across_tiles(pkg, geometry, metric):
    """identical sketches in three tiles (value 1.0) and 1/2 = 2/4 = 3/6 in three tiles: k cuts through both groups at the
    first, the middle and the last member"""
    tile = geometry[1]
    n = 2 * tile + 3
    query = [1, 2, 3, 100, 101]
    sketches = [[1000 + i] for i in range(n)]                  # the others share nothing with the query
    for i in (5, tile + 6, 2 * tile + 2):
        sketches[i] = list(query)
    sketches[9] = [1, 2, 3, 5000]                              # 3/4
    sketches[7] = [1, 6000]                                    # 1/2
    sketches[tile + 1] = [1, 2, 6001, 6002]                    # 2/4
    sketches[2 * tile + 1] = [1, 2, 3, 6003, 6004, 6005]       # 3/6
    index = build(pkg, sketches)
    qs = [mk(pkg, query), mk(pkg, [1, 6000])]
    for k in range(1, 9):
        got = check(pkg, sketches, [query, [1, 6000]], k, metric, index=index, qs=qs)
        if metric == SR.CONTAINMENT_NODE:
            assert [r[0] for r in got[0]] == [5, tile + 6, 2 * tile + 2, 9, 7, tile + 1, 2 * tile + 1][:k]
    assert SR.value(SR.CONTAINMENT_NODE, 1, 5, 2) == SR.value(SR.CONTAINMENT_NODE, 2, 5, 4) == SR.value(SR.CONTAINMENT_NODE, 3, 5, 6)


def test_rounded_fractions_tie_as_doubles(pkg):
    """two different fractions whose quotients are the same double: the node decides"""
    # 1/3 and 2/6 are the same double; so are 3/9 -- and 1/(2^53 + 1)-like cases need sizes no sketch has
    sketches = [[1, 2, 3, 10, 11, 12, 13, 14, 15], [1, 20, 21], [1, 2, 30, 31, 32, 33]]
    got = check(pkg, sketches, [[1, 2, 3]], 3, SR.CONTAINMENT_NODE)
    assert [r[0] for r in got[0]] == [0, 1, 2] and len({SR.value(SR.CONTAINMENT_NODE, r[1], r[3], r[2]) for r in got[0]}) == 1
    assert [r[0] for r in check(pkg, sketches[::-1], [[1, 2, 3]], 2, SR.CONTAINMENT_NODE)[0]] == [0, 1]


# ---------------------------------------------------------------------------------- one tile

@pytest.mark.parametrize("which", ["k=1", "k=max"])
def test_survivors_in_one_tile(pkg, geometry, which):
    """0, 1, k - 1, k, k + 1 survivors and the whole tile, scattered over the tile's waves"""
    max_k, tile, _ = geometry
    k = 1 if which == "k=1" else max_k
    counts = sorted({c for c in (1, k - 1, k, k + 1, tile) if c > 0})
    assert tile % 37 and counts[-1] == tile
    # node i holds hash 100 + c when its scattered position is below c, and up to two hashes of its own
    sketches = [[100 + c for c in counts if (i * 37) % tile < c] + [10_000 + 3 * i + j for j in range(i % 3)] for i in range(tile)]
    queries = [[100 + c] for c in counts] + [[99], [100 + c for c in counts]]
    for metric in (SR.JACCARD, SR.CONTAINMENT_QUERY):
        got = check(pkg, sketches, queries, k, metric)
        assert [len(g) for g in got] == [min(c, k) for c in counts] + [0, k]


@pytest.mark.parametrize("shape", ["tile-1", "tile", "tile+1", "2tile+1"])
def test_node_tile_edges(pkg, geometry, shape):
    max_k, tile, _ = geometry
    n = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2tile+1": 2 * tile + 1}[shape]
    # everybody holds 1; the last node, and the nodes at the edges of a wave's 64 nodes, hold 2 as well: they are the best
    edge = {i for i in (0, 63, 64, 255, 256, tile - 1, tile, n - 1) if i < n}
    sketches = [[1] + ([2] if i in edge else []) + [10 + 2 * i + j for j in range(i % 2)] for i in range(n)]
    index = build(pkg, sketches)
    queries = [[1, 2], [2], [1]]
    qs = [mk(pkg, q) for q in queries]
    for k in (3, len(edge), max_k):
        got = check(pkg, sketches, queries, k, SR.JACCARD, index=index, qs=qs)
        assert {r[0] for r in got[0][:len(edge)]} <= edge and len(got[2]) == min(k, n)
    assert {r[0] for r in got[1]} == edge


# ---------------------------------------------------------------------------------- merge steps

def test_merge_steps(pkg, geometry):
    """queries whose kept candidates total step - 1, step, step + 1 and two steps + 1 (step = merge_slots - k), k = max_k: every
    node up to a bound shares a hash with the query, so a whole tile keeps k candidates"""
    max_k, tile, slots = geometry
    k, step = max_k, slots - max_k
    totals = (step - 1, step, step + 1, 2 * step + 1)

    def nodes_for(total):                                      # whole tiles keep k each, the last tile the rest
        return (total // k) * tile + total % k

    bounds = [nodes_for(t) for t in totals]
    assert bounds == sorted(bounds) and all(tile >= k for _ in bounds)
    n = bounds[-1]
    shared_hash = [1 << 40, 2 << 40, 3 << 40, 4 << 40]
    best = 5 << 40                                             # held by the very last node alone: the candidate of the last step wins
    sketches = [[h for h, b in zip(shared_hash, bounds) if i < b] + [10 + 3 * i + j for j in range((i * 7) % 3)] for i in range(n)]
    sketches[n - 1] = [shared_hash[3], best]
    queries = [[h] for h in shared_hash[:3]] + [[shared_hash[3], best]]
    index = build(pkg, sketches)
    qs = [mk(pkg, q) for q in queries]
    shared = SR.shared(sketches, queries)
    assert [sum(min(k, sum(1 for r in rows if r[0] // tile == t)) for t in range(-(-n // tile))) for rows in shared] == list(totals)
    for metric in (SR.JACCARD, SR.CONTAINMENT_NODE):
        got = run(index, qs, k, metric)
        assert got == NR.select(shared, k, metric, 0.0), metric
        assert [len(g) for g in got] == [k] * 4 and (metric != SR.JACCARD or got[3][0] == (n - 1, 2, 2, 2))
    # a smaller k over the same candidates: fewer kept per tile, one step
    assert run(index, qs, 7, SR.JACCARD) == NR.select(shared, 7, SR.JACCARD, 0.0)


# ---------------------------------------------------------------------------------- the order of the values

@pytest.mark.parametrize("metric", [SR.JACCARD, SR.CONTAINMENT_NODE, SR.MAX_CONTAINMENT])
def test_value_order_over_binades(pkg, metric):
    """1.0, 2/3, 1/2, 1/3 and 1/1000 in one query: the bit patterns order as the values (containment_query has one
    denominator per query: its sizes cannot produce these)"""
    x = iter(range(10_000, 20_000))
    fill = lambda m: [next(x) for _ in range(m)]
    if metric == SR.JACCARD:                                   # common / (2 + size - common)
        query = [1, 2]
        by_value = {1.0: [1, 2], 2 / 3: [1, 2] + fill(1), 1 / 2: [1], 1 / 3: [1] + fill(1), 1 / 1000: [1] + fill(998)}
    elif metric == SR.CONTAINMENT_NODE:                        # common / size
        query = [1, 2, 3]
        by_value = {1.0: [1], 2 / 3: [1, 2] + fill(1), 1 / 2: [1] + fill(1), 1 / 3: [1] + fill(2), 1 / 1000: [1] + fill(999)}
    else:                                                      # common / min(1000, size)
        query = list(range(1, 1001))
        by_value = {1.0: [1], 2 / 3: [1, 2] + fill(1), 1 / 2: [1] + fill(1), 1 / 3: [1] + fill(2), 1 / 1000: [1] + fill(1500)}
    order = [1 / 3, 1.0, 1 / 1000, 2 / 3, 1 / 2]               # the nodes' order is not the values'
    sketches = [by_value[v] for v in order] + [fill(3)]
    got = check(pkg, sketches, [query], 5, metric)
    assert [SR.value(metric, c, lq, ls) for _, c, ls, lq in got[0]] == [1.0, 2 / 3, 1 / 2, 1 / 3, 1 / 1000]
    assert [r[0] for r in got[0]] == [1, 3, 4, 0, 2]
    assert [r[0] for r in check(pkg, sketches, [query], 2, metric)[0]] == [1, 3]


# ---------------------------------------------------------------------------------- chunks

def budgets_of(n, nq):
    return (n, 3 * n, nq * n)                                  # chunks of one query, of three queries, the whole batch


def test_chunk_budgets_change_no_result(pkg, fx):
    L = pkg.lib()
    n, nq = len(fx.mins), 20
    qs, sizes = fx.queries[:nq], [len(q) for q in fx.q_hashes[:nq]]
    exp = fx.expected(3, SR.JACCARD, 0.0)[:nq]
    assert run(fx.index, qs, 3, SR.JACCARD) == exp             # (the blocks of the shapes below are in the pool now)
    try:
        for budget in budgets_of(n, nq):
            pkg.matrix.set_search_many_budget(budget)
            for again in (False, True):
                pool = L.smh_pool_bytes()
                before = count(pkg, "nearest_chunk")
                assert run(fx.index, qs, 3, SR.JACCARD) == exp, budget
                assert count(pkg, "nearest_chunk") - before == len(SR.cut_chunks(sizes, n, budget)), budget
                assert not again or L.smh_pool_bytes() == pool, budget
    finally:
        pkg.matrix.set_search_many_budget(0)
    assert [len(SR.cut_chunks(sizes, n, b)) for b in budgets_of(n, nq)] == [20, 7, 1]


# ---------------------------------------------------------------------------------- other shapes

def test_other_shapes(pkg, geometry):
    sketches = [[1, 2, 3], [3, 4], [], [7, 8, 9, 10]]
    index = build(pkg, sketches)
    a, b = [1, 2, 3, 4], [8, 9, 11]
    for queries in ([[], a, b], [a, b, []], [a, [], [], b], [a, a], [a, b, a, b], [[]], [[], []]):
        for metric in SR.METRICS:
            for k in (1, 2, 100, geometry[0]):                 # k > n: every row, in order
                got = check(pkg, sketches, queries, k, metric, index=index)
                for q, rows in zip(queries, got):
                    assert rows == got[queries.index(q)]       # the same sketch gives the same rows
    res = index.nearest([], 3)
    assert len(res) == 0 and res.offsets.tolist() == [0]
    empty = pkg.index.ResidentIndex([])
    assert run(empty, [mk(pkg, a), mk(pkg, [])], 3, SR.JACCARD) == [[], []]
    assert len(empty.knn(3)) == 0 and empty.knn(3).offsets.tolist() == [0]
    hollow = build(pkg, [[], []])
    assert run(hollow, [mk(pkg, a)], 3, SR.CONTAINMENT_NODE) == [[]] and per_query(hollow.knn(3)) == [[], []]
    assert run(index, [mk(pkg, [20, 21])], 3, SR.JACCARD, -1.0) == [[]], "a pair that shares nothing is never a neighbour"
    assert run(index, [mk(pkg, a)], 3, SR.JACCARD, -1.0) == run(index, [mk(pkg, a)], 3, SR.JACCARD, 0.0)
    assert run(index, [mk(pkg, a)], 3, SR.JACCARD, 0.0, 2) == NR.nearest(sketches, [a], 3, SR.JACCARD, 0.0, 2) == [[(0, 3, 3, 4), (1, 2, 2, 4)]]


# ---------------------------------------------------------------------------------- the index against itself

def test_knn_of_a_path_graph(pkg):
    """200 nodes, node i shares one hash with node i - 1 and one with node i + 1"""
    n = 200
    sketches = [[i, i + 1] + [1000 + i] * (i % 2) for i in range(n)]
    index = build(pkg, sketches)
    exp = {k: NR.nearest_self(sketches, k, SR.JACCARD, 0.0) for k in (1, 2, 5)}
    assert [len(r) for r in exp[5]] == [1] + [2] * (n - 2) + [1]
    try:
        for budget in budgets_of(n, n):
            pkg.matrix.set_search_many_budget(budget)
            for k in exp:
                before = count(pkg, "nearest_chunk")
                got = per_query(index.knn(k))
                assert got == exp[k], (budget, k)
                assert count(pkg, "nearest_chunk") - before == len(SR.cut_chunks([len(s) for s in sketches], n, budget))
                assert all(r[0] != q for q, rows in enumerate(got) for r in rows), "node == query is never reported"
    finally:
        pkg.matrix.set_search_many_budget(0)


def test_knn_of_the_fixture_and_of_a_downsampled_index(fx):
    for metric in (SR.JACCARD, SR.CONTAINMENT_NODE):
        got = per_query(fx.index.knn(4, NAMES[metric], 0.01))
        assert got == NR.nearest_self(fx.mins, 4, metric, 0.01) and sum(map(len, got)) > 100
        assert all(r[0] != q for q, rows in enumerate(got) for r in rows)
    cut_at = fx.max_hash // 4
    child = fx.index.downsample(max_hash=cut_at)
    assert len(child.nodes[0]) == len(fx.mins[0]), "the Python nodes of a downsampled index are the uncut sketches"
    cut = [[h for h in m if h <= cut_at] for m in fx.mins]
    for metric, thr_bp in ((SR.JACCARD, 0), (SR.CONTAINMENT_QUERY, 3 * round(2 ** 64 / cut_at))):
        got = per_query(child.knn(3, NAMES[metric], threshold_bp=thr_bp))
        assert got == NR.nearest_self(cut, 3, metric, 0.0, 3 if thr_bp else 0) and sum(map(len, got)) > 20


def test_nearest_downsample_groups_the_queries(pkg, fx):
    cut_at = fx.max_hash // 4
    cut = [[h for h in m if h <= cut_at] for m in fx.mins]
    many = per_query(fx.index.nearest([mk(pkg, m, max_hash=cut_at) for m in cut[:7]] + fx.queries[7:12], 2, downsample=True))
    assert many[:7] == NR.nearest(cut, cut[:7], 2, SR.JACCARD, 0.0) and many[7:] == fx.expected(2, SR.JACCARD, 0.0)[7:12]


# ---------------------------------------------------------------------------------- the other forms

def test_csr_device_form_on_the_callers_stream(pkg, fx):
    import torch
    flat, off = pkg.matrix.csr_from_sketches([np.array(sorted(q), dtype=np.uint64) for q in fx.q_hashes])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(flat.view(np.int64)).cuda()
    stream.synchronize()
    for metric, threshold, thc, k in ((SR.JACCARD, 0.1, 0, 3), (SR.MAX_CONTAINMENT, 0.0, 25, 100)):
        exp = NR.select(fx.shared, k, metric, threshold, thc)
        for handle in (stream.cuda_stream, None):
            res = fx.index.nearest_block_dev(t.data_ptr(), off, k, NAMES[metric], threshold, threshold_common=thc, stream=handle)
            assert per_query(res) == exp
    # an offset that is not 0: the batch is its tail
    res = fx.index.nearest_block_dev(t.data_ptr(), off[90:], 3, "jaccard", 0.1)
    assert per_query(res) == fx.expected(3, SR.JACCARD, 0.1)[90:]
    # a CSR carries no parameters: an index that does not speak with one voice is refused
    odd = pkg.index.ResidentIndex([mk(pkg, fx.mins[0], max_hash=fx.max_hash), mk(pkg, fx.mins[1], max_hash=fx.max_hash, seed=43)])
    with pytest.raises(pkg.SourmashError) as ei:
        odd.nearest_block_dev(t.data_ptr(), off, 3)
    assert ei.value.code == 3 and "same ksize" in ei.value.message


def test_queries_resident_on_the_device(pkg, pyoracle):
    mx = M64 // 20
    genome = pyoracle.synth_dna(0, 30000, 21)
    parts = [genome[a:b] for a, b in ((0, 12000), (8000, 20000), (15000, 30000), (0, 30000))]

    def sketched(part):
        mh = pkg.KmerMinHash(0, 21, False, 42, mx, False)
        mh.add_sequence(part, True)
        return mh

    nodes = [sketched(genome[a:a + 4000]) for a in range(0, 30000, 3000)]
    node_mins = [m.mins for m in nodes]
    index = pkg.index.ResidentIndex(nodes)
    hosts = [mk(pkg, t.mins, max_hash=mx) for t in [sketched(p) for p in parts]]
    resident = [sketched(p) for p in parts]
    batch = [resident[0], hosts[1], resident[2], resident[3]]              # HBM and host states in one batch
    before = count(pkg, "sketch_to_host")
    got = run(index, batch, 3, SR.CONTAINMENT_NODE)
    assert count(pkg, "sketch_to_host") == before, "nearest brought a device-resident query to the host"
    assert got == run(index, hosts, 3, SR.CONTAINMENT_NODE) == NR.nearest(node_mins, [h.mins for h in hosts], 3, SR.CONTAINMENT_NODE, 0.0)
    assert [len(g) for g in got] == [3] * 4
    assert resident[0].mins == hosts[0].mins                   # they were resident: looking at one moves it now
    assert count(pkg, "sketch_to_host") == before + 1


# ---------------------------------------------------------------------------------- the kernels and the test knobs

def test_the_kernels_ran(pkg):
    L = pkg.lib()
    index = build(pkg, [[1, 2, 3], [3, 4]])
    qs = [mk(pkg, [1, 2, 3, 4]), mk(pkg, [4])]
    names = ("search_many_probe", "search_many_select", "nearest_clamp", "nearest_tile", "nearest_merge", "search_many_emit")
    L.smh_profile_enable(1)
    try:
        L.smh_profile_reset()
        assert run(index, qs, 1, SR.JACCARD) == [[(0, 3, 3, 4)], [(1, 1, 2, 1)]]
        assert [count(pkg, k) for k in names] == [1, 1, 1, 1, 1, 0]
        assert per_query(index.knn(2)) == [[(1, 1, 2, 3)], [(0, 1, 3, 2)]]
        assert [count(pkg, k) for k in names] == [2, 2, 2, 2, 2, 0]
        assert run(index, qs, 1, SR.JACCARD, 1.0) == [[], []]  # nothing survives: no candidates, no rows
        assert [count(pkg, k) for k in names] == [3, 3, 3, 2, 2, 0]
    finally:
        L.smh_profile_enable(0)


def test_pool_fill_and_grid_caps_change_no_result(pkg, fx, geometry):
    L = pkg.lib()
    cases = [(3, SR.JACCARD, 0.0), (geometry[0], SR.CONTAINMENT_QUERY, 0.1)]

    def all_cases():
        for k, metric, threshold in cases:
            assert per_query(fx.index.nearest(fx.queries, k, NAMES[metric], threshold)) == fx.expected(k, metric, threshold)
        assert per_query(fx.index.knn(4, "jaccard", 0.01)) == NR.nearest_self(fx.mins, 4, SR.JACCARD, 0.01)

    all_cases()
    try:
        pkg.matrix.set_pool_fill(TEST_BYTE)
        before = count(pkg, "pool_filled")
        all_cases()
        assert count(pkg, "pool_filled") > before
        pool = L.smh_pool_bytes()
        all_cases()
        assert L.smh_pool_bytes() == pool, "a call left a block out of the pool"
    finally:
        pkg.matrix.set_pool_fill(-1)
    try:
        for cap in (1, 2):
            pkg.matrix.set_grid_cap(cap)
            before = count(pkg, "grid_capped")
            all_cases()
            assert count(pkg, "grid_capped") > before
    finally:
        pkg.matrix.set_grid_cap(0)
    gc.collect()


# ---------------------------------------------------------------------------------- errors

def test_errors_write_nothing(pkg, geometry):
    L = pkg.lib()
    u64p = C.POINTER(C.c_uint64)
    max_k = geometry[0]
    nodes = [mk(pkg, [1, 2, 3]), mk(pkg, [3, 4])]
    index = pkg.index.ResidentIndex(nodes)
    good = [mk(pkg, [1, 2, 3, 4]) for _ in range(5)]
    assert [len(r) for r in run(index, good, 2, SR.JACCARD)] == [2] * 5

    def raw(idx, queries, k=2, metric=0, threshold=0.1, null_rows=False, null_offsets=False):
        arr = (C.c_void_p * len(queries))(*[q._p for q in queries])
        row_off = np.full(len(queries) + 1, SENTINEL, dtype=np.uint64)
        rows_p = C.POINTER(pkg._lib.SmhSearchRow)()
        L.sourmash_err_clear()
        rc = L.smh_index_nearest_many(idx._h, arr, len(queries), k, metric, threshold, 0, None if null_offsets else row_off.ctypes.data_as(u64p),
                                      None if null_rows else C.byref(rows_p))
        assert rc != 0 and not rows_p and (row_off == SENTINEL).all()
        with pytest.raises(pkg.SourmashError) as ei:
            pkg.errors.check()
        assert ei.value.code == rc
        return ei.value

    for k in (0, max_k + 1):
        e = raw(index, good, k=k)
        assert e.code == 3 and str(max_k) in e.message
        with pytest.raises(pkg.SourmashError) as ei:
            index.knn(k)
        assert ei.value.code == 3 and str(max_k) in ei.value.message
    assert raw(index, good, threshold=float("nan")).code == 3 and raw(index, good, metric=4).code == 3
    assert "k is" not in raw(index, good, k=0, metric=4).message          # the metric is looked at first, as search_many does
    assert raw(index, good, null_rows=True).code == 1 and raw(index, good, null_offsets=True).code == 1
    e = raw(index, good[:3] + [mk(pkg, [1, 2], num=5)] + good[4:])
    assert e.code == 3 and "query 3" in e.message and "scaled" in e.message
    e = raw(index, [good[0], mk(pkg, [1, 2], ksize=31), good[2], mk(pkg, [1, 2], num=5), mk(pkg, [1, 2], seed=43)])
    assert e.code == 101 and "query 1" in e.message              # the lowest failing query, whatever the later ones are
    e = raw(index, [good[0], good[1], mk(pkg, [1, 2], seed=43), mk(pkg, [1, 2], ksize=31)])
    assert e.code == 104 and "query 2" in e.message
    mixed = pkg.index.ResidentIndex(nodes + [mk(pkg, [1, 2, 9], num=5)])
    e = raw(mixed, good)
    assert e.code == 3 and "query 0" in e.message and "num sketch" in e.message
    with pytest.raises(pkg.SourmashError) as ei:
        index.nearest(good[:2] + [mk(pkg, [1], max_hash=1 << 62)], 2, scaled=1)
    assert ei.value.code == 103 and "query 2" in ei.value.message
    for call in (lambda: mixed.knn(2), lambda: index.knn(2, threshold=float("nan")),
                 lambda: pkg.index.ResidentIndex(nodes + [mk(pkg, [5], seed=43)]).knn(2)):
        with pytest.raises(pkg.SourmashError) as ei:
            call()
        assert ei.value.code in (3, 104)
    assert [len(r) for r in run(index, good, 2, SR.JACCARD)] == [2] * 5, "a refusal leaves the index usable"
