"""The grid-stride loops of the resident-index kernels (gather, gather_many, search_many / search_self, cluster, match, lca,
collapse, index build) on their second and third trips.  The grids are min(ceil(items / items per workgroup), a limit of
hundreds of workgroups), so at the sizes of the other test files every loop runs once; smh_set_grid_cap lowers the grids
instead of raising the sizes.  Every operation runs the same small input under the caps 1 (one workgroup takes every trip),
3 (workgroups take different numbers of trips, the last trip part-filled) and 0 (the default), and every result must EQUAL
the plain-Python restatement -- all outputs are integers or rule-defined doubles.  Cap 2 runs as well: a kernel with a lane
per item has a default grid of 3 at 700 items, which cap 3 does not lower; under cap 2 its first workgroup takes a second,
part-filled trip and the other does not.  The event counter "grid_capped" must rise under the caps 1, 2 and 3 and stand
still under 0: the caps really lowered grids.  The shapes read the kernels' branch sizes from
the *_geometry() calls; the trips they reach are in each test's docstring (a workgroup is 256 threads, 4 waves).

Two tests at the end need no cap: the subtract kernels of gather and gather_many have constant grid limits (256 and 32
workgroups), and a winner with 70 000 hits passes both."""
import random

import numpy as np
import pytest

import cluster_restatement as CR
import collapse_restatement as CO
import gather_restatement as GR
import index_build_restatement as IB
import lca_restatement as LR
import match_restatement as MR
import search_many_restatement as SR
import test_gpu_cluster as TC
import test_gpu_collapse as TCO
import test_gpu_gather as TG
import test_gpu_gather_many as TGM
import test_gpu_index_build as TIB
import test_gpu_lca as TL
import test_gpu_match as TM
import test_gpu_search_many as TS

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
CAPS = (1, 2, 3, 0)
GATHER_SHORT_LIST = 8   # kGatherShortList of gather_kernels.hip (no geometry call reports it; the test plants a list of 10)
mk, count = TG.mk, TG.count


@pytest.fixture
def grid(pkg):
    """sets the grid cap; the default is back when the test ends, however it ends"""
    try:
        yield pkg.matrix.set_grid_cap
    finally:
        pkg.matrix.set_grid_cap(0)


def under_caps(pkg, grid, fn, at_least=1):
    """fn(cap) under every cap; the cap 1 lowered at least `at_least` grids, the caps 2 and 3 one at least, the cap 0 none"""
    out = []
    for cap in CAPS:
        grid(cap)
        assert pkg.matrix.grid_cap() == cap
        before = count(pkg, "grid_capped")
        out.append(fn(cap))
        moved = count(pkg, "grid_capped") - before
        assert moved >= {1: at_least, 2: 1, 3: 1}[cap] if cap else moved == 0, (cap, moved)
    return out


# ---------------------------------------------------------------------------------- gather, gather_many, search_many, search_self

class Nodes:
    """A query of 1 500 hashes and n >= 11 nodes over a pool of 3 000 hashes.  The sizes begin 0, 1, 64, 65, 130, 900 (a node of
    one step, of one step and one element, of three steps: base and cc carry from step to step).  Node 5 holds 900 query
    hashes: the winner of round 0.  The three largest hashes of the pool are in the query: `shared` is held by the nodes 1 .. 10
    (an inverted list of 10 > kGatherShortList; it is the last entry of the winner's hit list), `p_short` and `p_long` by
    `short` and `short + 1` nodes (the owner lists on both sides of kShortOwners)."""

    def __init__(self, n, short):
        assert n >= 11 and short + 1 <= 9 and GATHER_SHORT_LIST < 10
        rng = np.random.default_rng(101 + n)
        pool = sorted(set(int(x) for x in rng.integers(1, M64 - 10, 3003, dtype=np.uint64)))[:3003]
        self.p_short, self.p_long, self.shared = pool[-3:]
        pool = pool[:-3]
        inside, outside = pool[0::2], pool[1::2]
        self.query = sorted(inside[:1497] + [self.shared, self.p_short, self.p_long])
        self.outside = outside
        sizes = [0, 1, 64, 65, 130, 900, 300, 200, 129, 63, 128] + [int(x) for x in rng.integers(0, 150, n - 11)]
        self.sketches = []
        for v, size in enumerate(sizes):
            held = set()
            if 1 <= v <= 10:
                held.add(self.shared)
            if 2 <= v < 2 + short:
                held.add(self.p_short)
            if 2 <= v < 3 + short:
                held.add(self.p_long)
            rest = size - len(held)
            k = rest if v == 5 else rest // 2               # the winner lies inside the query; the others half outside
            held |= set(TG.pick(rng, inside[:1497], k)) | set(TG.pick(rng, outside, rest - k))
            assert len(held) == size, v
            self.sketches.append(sorted(held))
        self.ab = {h: 1 + h % 7 for h in self.query}
        self.winner = sorted(set(self.sketches[5]) & set(self.query))
        assert len(self.winner) > 768 and self.winner[-1] == self.shared     # more than three trips of 256 hits; the list of 10 in the last

    def index(self, pkg):
        return pkg.index.ResidentIndex([mk(pkg, s) for s in self.sketches])


@pytest.fixture(scope="module")
def short_owners(pkg):
    return pkg.matrix.search_geometry()[0]


@pytest.fixture(scope="module", params=[11, 29])
def nodes(request, short_owners):
    return Nodes(request.param, short_owners)


def test_gather(pkg, grid, nodes):
    """k_gather_hits, k_gather_invert (a wave per node): 11 nodes are 3 trips under cap 1, the last with one wave idle; 29 nodes
    are 3 trips under cap 3, in the last of which workgroup 0 is full, workgroup 1 holds one node and workgroup 2 none.
    k_gather_subtract (256 hits per workgroup and trip): the winner's 900 hits are 4 trips under cap 1 and 2 under cap 3 (the
    default grid is 4).  Abundances as none, as host pairs, as u64 counts in HBM and as the run starts of a bulk fold."""
    exp = {w: GR.gather(nodes.sketches, nodes.query, nodes.ab if w else None) for w in (True, False)}
    assert exp[True][0][0]["match"] == 5 and exp[True][0][0]["common_remaining"] == len(nodes.winner) and len(exp[True][0]) >= 5

    def run(cap):
        index = nodes.index(pkg)
        starts = pkg.KmerMinHash(0, 21, False, 42, M64, True)                # one bulk fold: hashes + run starts, in HBM
        starts.add_many(np.repeat(np.array(nodes.query, dtype=np.uint64), [nodes.ab[h] for h in nodes.query]))
        counts = mk(pkg, nodes.query, nodes.ab)                              # a host state moved to HBM: hashes + u64 counts
        assert counts.export_dev() == len(nodes.query)
        for q, w in ((mk(pkg, nodes.query), False), (mk(pkg, nodes.query, nodes.ab), True), (counts, True), (starts, True)):
            res = index.gather(q, threshold_bp=1, scaled=1, abund_stats=False)
            assert TG.as_dicts(res.rows) == exp[w][0], (cap, w)
            assert res.assigned.tolist() == exp[w][1], (cap, w)

    under_caps(pkg, grid, run, at_least=4)


class Batch:
    """5 queries against Nodes: 150 hashes, none, 170 (the last two of them p_short and p_long, which so sit in the second trip
    of the probe), 650 of the winner's hashes (one (query, node) with more than 600 hits) and 141.  1 111 positions: 5 trips
    under cap 1, 2 under cap 3; no query begins on a multiple of 256."""

    def __init__(self, nodes):
        rng = np.random.default_rng(7)
        some = lambda k: TG.pick(rng, nodes.query[:-3], k // 2) + TG.pick(rng, nodes.outside, k - k // 2)
        self.queries = [sorted(some(150)), [], sorted(some(168) + [nodes.p_short, nodes.p_long]), sorted(TG.pick(rng, nodes.winner[:-1], 650)),
                        sorted(some(141))]
        off = np.cumsum([0] + [len(q) for q in self.queries]).tolist()
        assert off == [0, 150, 150, 320, 970, 1111] and all(o % 256 for o in off[1:])
        assert 256 <= off[3] - 2 and off[3] <= 512
        self.abunds = [{h: 1 + h % 5 for h in q} for q in self.queries]


@pytest.fixture(scope="module")
def batch(nodes):
    return Batch(nodes)


def test_gather_many(pkg, grid, nodes, batch):
    """k_gm_probe, k_gm_fill (1 111 positions), k_gm_weights (the 650 run starts of a query in HBM: 3 trips under cap 1),
    k_gm_subtract (650 hits of one (query, node): 3 trips of its one workgroup)"""
    exp = {w: [GR.gather(nodes.sketches, q, a if w else None) for q, a in zip(batch.queries, batch.abunds)] for w in (True, False)}
    assert exp[False][3][0][0]["common_remaining"] == 650 and exp[False][1] == ([], [])

    def run(cap):
        index = nodes.index(pkg)
        flat = [mk(pkg, q) for q in batch.queries]
        weighted = [mk(pkg, q, a) for q, a in zip(batch.queries, batch.abunds)]
        assert weighted[0].export_dev() == 150                               # u64 counts in HBM
        q3, a3 = batch.queries[3], batch.abunds[3]
        weighted[3] = pkg.KmerMinHash(0, 21, False, 42, M64, True)           # run starts in HBM
        weighted[3].add_many(np.repeat(np.array(q3, dtype=np.uint64), [a3[h] for h in q3]))
        for qs, w in ((flat, False), (weighted, True)):
            res = index.gather_many(qs, threshold_bp=1, scaled=1, abund_stats=False)
            got = [(TGM.as_dicts(r.rows), r.assigned.tolist()) for r in res]
            assert got == exp[w], (cap, w)

    under_caps(pkg, grid, run, at_least=4)


@pytest.mark.parametrize("metric", SR.METRICS)
def test_search_many_and_search_self(pkg, grid, nodes, batch, metric):
    """k_sm_probe: the batch's 1 111 positions, and the index's own hashes as the queries of search_self"""
    shared = SR.shared(nodes.sketches, batch.queries)
    own = SR.shared(nodes.sketches, nodes.sketches)
    thresholds = (0.0, 0.04)
    exp = [SR.select(shared, metric, t) for t in thresholds]
    exp_self = {(t, up): [[r for r in rows if (r[0] > q if up else r[0] != q)] for q, rows in enumerate(SR.select(own, metric, t))]
                for t in thresholds for up in (True, False)}
    assert sum(map(len, exp[0])) > sum(map(len, exp[1])) > 0

    def run(cap):
        index = nodes.index(pkg)
        qs = [mk(pkg, q) for q in batch.queries]
        for t, want in zip(thresholds, exp):
            assert TS.per_query(index.search_many(qs, t, TS.NAMES[metric], scaled=1)) == want, (cap, t)
        for (t, up), want in exp_self.items():
            assert TS.per_query(index.pairwise(t, TS.NAMES[metric], upper=up)) == want, (cap, t, up)

    under_caps(pkg, grid, run, at_least=3)


# ---------------------------------------------------------------------------------- cluster

@pytest.mark.parametrize("n", [600, 1100])
@pytest.mark.parametrize("metric", [CR.JACCARD, CR.MAX_CONTAINMENT])
def test_cluster(pkg, grid, metric, n):
    """600 nodes of a few hashes: k_cl_round and k_cl_assign (a lane per node) take 3 trips under cap 1, and in the last one
    the waves of the lanes 640 .. 767 hold no node at all, the wave of 576 .. 639 a part of one.  1 100 nodes: 5 trips under
    cap 1, and 2 under cap 3, where workgroup 0 takes a full second trip, workgroup 1 a part of one and workgroup 2 none.  Two
    hubs sit in the last trip with adjacency lists longer than kClusterLaneMax, walked by their waves: node n - 50, first in
    priority, becomes a representative; node n - 10, last in priority and in the part-filled wave, becomes a member and
    chooses among its representatives by the butterfly.  Chains of descending priority take several rounds.  k_cl_probe
    walks the index's own hashes (components), a few thousand positions."""
    lane_max = pkg.matrix.cluster_geometry()[0]
    top, last = n - 50, n - 10
    rng = random.Random(5)
    others = [v for v in range(n) if v not in (top, last)]
    edges = [(top, u) for u in rng.sample(others, 2 * lane_max + 9)] + [(last, u) for u in rng.sample(others, lane_max + 1)]
    for a in range(0, 500, 25):
        edges += [(v, v + 1) for v in range(a, a + 6)]
    edges += [tuple(rng.sample(others, 2)) for _ in range(120)]
    sketches = TC.edge_sketches(n, edges)
    scores = [1 + (v * 37) % 101 for v in range(n)]
    scores[top], scores[last] = 1000, 0
    for a in range(0, 500, 25):                              # priority descends along every chain: a round decides one link
        for k in range(7):
            scores[a + k] = 500 - k
    exp = {link: CR.cluster(sketches, metric, 0.0, 0, link, scores) for link in (CR.COMPONENTS, CR.GREEDY)}
    greedy = exp[CR.GREEDY]
    assert greedy[1][top] == top and greedy[1][last] != last and 3 < exp[CR.COMPONENTS][3] < greedy[3] < n

    def run(cap):
        index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
        for link in (CR.COMPONENTS, CR.GREEDY):
            res = index.cluster(0.0, TC.NAMES[metric], TC.LINKS[link], scores=scores, scaled=1)
            assert TC.as_lists(res) == exp[link], (cap, link)

    under_caps(pkg, grid, run, at_least=4)


# ---------------------------------------------------------------------------------- match, lca_records

class Reads:
    """14 records of a synthetic genome: every window is sampled (max_hash 2^64 - 1) and distinct, so a record of length L is
    L - 20 runs.  The runs of record 4 straddle run 256, those of record 6 the runs 512 and 768: the probe's segmented
    scan joins them across trips only by its atomics.  24 nodes; the first hits[r] windows of record r are held by owners[r]
    nodes each, so the owner pairs are hits * owners: records 0, 1, 3, 4, 7, 8, 10, 12, 13 reach the tally's LDS regime
    with different counts, record 6 is dense (more than kMatchLdsPairs; its 560 runs are 3 trips of the one workgroup that
    k_match_dense_count has per record under cap 1), record 9 hits nothing, record 11 has no window.  Under cap 1 wave w of the
    tally takes the records w, w + 4, w + 8, w + 12: record 5 (3 pairs) follows record 1 (900 pairs) in the same LDS slice.
    11 records have more than kLcaRecordLaneMax runs: 3 trips of k_lca_records_long under cap 1."""
    RUNS = [40, 100, 5, 90, 60, 3, 560, 70, 80, 9, 50, 0, 60, 30]
    HITS = [40, 100, 5, 70, 60, 3, 560, 33, 80, 0, 50, 0, 60, 11]
    OWNERS = [5, 9, 2, 11, 2, 1, 12, 7, 12, 0, 3, 0, 1, 24]

    def __init__(self, pyoracle, lds_pairs, record_lane_max):
        genome = pyoracle.synth_dna(0, 4000, 77)
        self.records, at = [], 0
        for runs in self.RUNS:
            length = runs + 20 if runs else 10
            self.records.append(genome[at:at + length])
            at += length + 30
        ws = [MR.window_hashes(r, 21) for r in self.records]
        assert [len(set(w)) for w in ws] == self.RUNS and len(set(h for w in ws for h in w)) == sum(self.RUNS)
        first = np.cumsum([0] + self.RUNS).tolist()
        assert first[4] < 256 < first[5] and first[6] < 512 and 768 < first[7] and sum(self.RUNS) == 1157
        n = 24
        self.nodes = [[] for _ in range(n)]
        for r, w in enumerate(ws):
            for i, h in enumerate(w[:self.HITS[r]]):
                for t in range(self.OWNERS[r]):
                    self.nodes[(r + t + i * 5 % 7) % n].append(h)
        self.nodes[23] += TM.unrelated(random.Random(2), 40)
        pairs = [h * o for h, o in zip(self.HITS, self.OWNERS)]
        assert max(pairs) == pairs[6] > lds_pairs and sorted(pairs)[-2] <= lds_pairs and pairs[1] > 100 * pairs[5] > 0
        assert len(set(p for p in pairs if 0 < p <= lds_pairs)) >= 9
        assert sum(1 for runs in self.RUNS if runs > record_lane_max) >= 9
        rng = random.Random(9)
        self.parent = TL.bushy(rng, 60)
        self.node_taxon = [rng.randrange(60) if v % 5 else TL.NO for v in range(n)]
        # 600 reads of one to four windows from 150 places: the kernels with a lane per record take 3 trips under cap 1
        self.short = [genome[(k * 7) % 150 * 20:(k * 7) % 150 * 20 + 21 + k % 4] for k in range(600)]


@pytest.fixture(scope="module")
def reads(pkg, pyoracle):
    return Reads(pyoracle, pkg.matrix.match_geometry()[0], pkg.matrix.lca_geometry()[1])


def test_match(pkg, grid, reads):
    """k_match_owner_ids (the directory is built under the cap: a new index per cap), k_match_probe, k_match_tally,
    k_match_dense_count, k_match_hit_scatter: rows and hit lists"""
    owners = MR.owners_of(reads.nodes)
    exp = {name: MR.match(recs, 21, 42, M64, owners) for name, recs in (("long", reads.records), ("short", reads.short))}
    rows = exp["long"][0]
    assert rows[6][4] != MR.MISS and rows[9][2:] == (0, 0, MR.MISS, 0) and rows[11] == (0, 0, 0, 0, MR.MISS, 0)
    assert sum(r[3] for r in exp["short"][0]) > 300

    def run(cap):
        index = TM.make_index(pkg, reads.nodes)
        for name, recs in (("long", reads.records), ("short", reads.short)):
            res = index.match(recs, hits=True)
            assert TM.rows_of(res) == exp[name][0], (cap, name)
            assert res.hit_offsets.tolist() == exp[name][1] and res.hit_hashes.tolist() == exp[name][2], (cap, name)
            assert TM.rows_of(index.match(recs)) == exp[name][0], (cap, name)

    under_caps(pkg, grid, run, at_least=6)


def test_lca_records(pkg, grid, reads):
    """k_lca_records (a lane per record: the 600 short reads) and k_lca_records_long (a wave per record), behind match's probe"""
    owners = MR.owners_of(reads.nodes)
    exp = {name: LR.classify_records(reads.parent, reads.node_taxon, owners, recs, 21, 42, M64)
           for name, recs in (("long", reads.records), ("short", reads.short))}
    assert len({r[5] for r in exp["long"]}) == 3 and len({r[4] for r in exp["long"]}) > 3

    def run(cap):
        index = TL.make_index(pkg, reads.nodes, reads.parent, reads.node_taxon)
        for name, recs in (("long", reads.records), ("short", reads.short)):
            assert TL.rows_of(index.lca_classify_records(recs)) == exp[name], (cap, name)

    under_caps(pkg, grid, run, at_least=4)


# ---------------------------------------------------------------------------------- lca: the table and the sketch route

@pytest.mark.parametrize("shape", ["chain", "branching"])
def test_lca_table_and_lca_many(pkg, grid, shape):
    """A directory of 700 ranks over 30 nodes: k_lca_table (a lane per rank) takes 3 trips under cap 1; every fifth rank has
    more than kLcaOwnerLaneMax owners -- 140 lists for k_lca_table_long, a wave each.  5 queries, one empty, 724 positions:
    k_lca_probe and k_lca_keys.  The table is made by the first call on an index: a new index per cap."""
    lane = pkg.matrix.lca_geometry()[0]
    rng = random.Random(31)
    parent = TL.chain(21) if shape == "chain" else TL.bushy(rng, 200)
    n = 30
    node_taxon = [rng.randrange(len(parent)) if v % 6 else TL.NO for v in range(n)]
    hashes = TL.unrelated(rng, 700)
    lengths = [1, 2, lane, lane + 1, 3, 1, lane + 4, 2, 1, 2 * lane + 3]
    nodes = [[] for _ in range(n)]
    for k, h in enumerate(hashes):
        for v in rng.sample(range(n), lengths[k % 10]):
            nodes[v].append(h)
    assert sum(1 for k in range(700) if lengths[k % 10] > lane) >= 9
    foreign = TL.unrelated(random.Random(32), 60)
    queries = [rng.sample(hashes, 150), [], rng.sample(hashes, 130) + foreign[:30], rng.sample(hashes, 283), rng.sample(hashes, 101) + foreign[30:]]
    assert sum(map(len, queries)) == 724
    owners = LR.owners_of(nodes)
    exp = [LR.counts(parent, node_taxon, owners, q) for q in queries]
    assert len(exp[0][0]) > 3 and exp[1] == ([], [])

    def run(cap):
        index = TL.make_index(pkg, nodes, parent, node_taxon)
        got = index.lca_counts([TL.sketch(pkg, q) for q in queries], hash_taxon=True)
        for k, ((taxa, cnt, per), (pairs, want_per)) in enumerate(zip(got, exp)):
            assert per.tolist() == want_per, (cap, k)
            assert list(zip(taxa.tolist(), cnt.tolist())) == pairs, (cap, k)

    under_caps(pkg, grid, run, at_least=4)


# ---------------------------------------------------------------------------------- collapse

class Owned:
    """300 nodes of two private hashes each and 100 planted hashes: 700 ranks, 3 trips of k_collapse_lane under cap 1.  The
    planted owner lists: 14 of different lengths from kCollapseLaneMax + 1 to kCollapseWaveMax, long and short by turns
    (k_collapse_wave, 4 per workgroup: a short list inherits the LDS scratch of a long one), 3 longer than kCollapseWaveMax
    (k_collapse_long: 3 trips of one workgroup under cap 1), the others up to kCollapseLaneMax.  Abundances: 1 + (v + hash) % 5."""

    def __init__(self, lane_max, wave_max):
        self.n = n = 300
        assert lane_max + 6 < 33 < wave_max - 6 and wave_max + 43 <= n
        mids = [wave_max, lane_max + 1, wave_max - 6, lane_max + 2, wave_max // 2, lane_max + 4, 64, 65, lane_max + 1 + 2, wave_max - 1,
                33, 100, lane_max + 6, 200]
        longs = [wave_max + 1, wave_max + 24, n]
        lengths = mids + longs + [1 + k % lane_max for k in range(100 - len(mids) - len(longs))]
        assert len(set(mids)) == len(mids) >= 9 and len(lengths) == 100
        rng = random.Random(13)
        order = list(range(100))
        rng.shuffle(order)                                   # the planted hashes ascend in this order: the regimes are mixed along the ranks
        held = [[(1 << 40) + 4 * v, (1 << 62) + 4 * v + 1] for v in range(n)]
        for place, k in enumerate(order):
            h = (1 << 50) + (place << 20) + lengths[k]
            start = (k * 7) % n
            for i in range(lengths[k]):
                held[(start + i) % n].append(h)
        self.sketches = [[(h, 1 + (v + h) % 5) for h in hs] for v, hs in enumerate(held)]
        self.ranks = 2 * n + 100


@pytest.fixture(scope="module")
def owned(pkg):
    lane_max, wave_max, _ = pkg.matrix.collapse_geometry()
    return Owned(lane_max, wave_max)


@pytest.mark.parametrize("abund", ["flat", "sum", "count"])
def test_collapse(pkg, grid, owned, abund):
    """Three groupings: groups spread over more than two kCollapseGroupTile (the long lists visit three tiles of LDS counters),
    two nodes per group and min_count 2 (the ranks with one member of a group fail); seven groups with every ninth node
    dropped and min_count 20 (the short lists fail, the long ones pass in part); one group and min_fraction 0.5.
    k_collapse_bounds has a lane per group, k_collapse_finish one per survivor."""
    tile = pkg.matrix.collapse_geometry()[2]
    n, G = owned.n, 2 * tile + 5
    cases = [([(v // 2) * 27 + 75 for v in range(n)], G, 2, 0.0),
             ([None if v % 9 == 4 else v % 7 for v in range(n)], 7, 20, 0.0),
             ([0] * n, 1, 1, 0.5)]
    spread = [g for g in cases[0][0]]
    assert min(spread) < tile and 2 * tile <= max(spread) < G
    src = owned.sketches if abund == "sum" else TCO.flat(owned.sketches)
    exp = [CO.collapse(src, group, g, mc, mf, TCO.MODES[abund]) for group, g, mc, mf in cases]
    sizes = [len(e[1]) for e in exp]
    assert owned.ranks < sizes[0] < sum(map(len, owned.sketches)) and 0 < sizes[1] < owned.ranks and 0 < sizes[2] < 10   # (group, hash) survivors

    def run(cap):
        index = TCO.index_of(pkg, owned.sketches)
        for (group, g, mc, mf), want in zip(cases, exp):
            TCO.same(index.collapse(group, g, mc, mf, abund), want, "cap %d G=%d" % (cap, g))

    under_caps(pkg, grid, run, at_least=6)


# ---------------------------------------------------------------------------------- index build, concat

def test_index_build_and_concat(pkg, grid):
    """14 records in 11 groups, 760 windows in about 690 runs: k_ib_counts and k_ib_finish (a lane per run) take 3 trips under cap 1.  600 short
    records, a node each: k_ib_groups (a lane per record) and the bisections of k_ib_finish (a lane per group) take 3.
    concat of three parts: k_ib_rebase over the 601 offsets of a part."""
    rng = np.random.default_rng(41)
    like = TIB.like_of(pkg, 21)
    lens = [70, 90, 20, 64, 85, 40, 33, 120, 41, 75, 21, 60, 95, 226]
    assert sum(n - 20 for n in lens) == 760
    records = [TIB.dna(rng, n) for n in lens]
    records[7] = records[1][:60] + records[7][60:]           # a stretch shared by two groups and repeated inside one
    records[12] = records[1][:50] + records[12][50:]
    groups = [3, 0, 1, 4, 2, 1, 5, 0, 6, 3, 7, 8, 0, 10]    # group 9 stays empty
    many = [TIB.dna(rng, 21 + k % 4) for k in range(600)]
    p = TIB.params(like)
    exp = IB.build(records, groups, 11, p)
    exp_many = IB.build(many, None, 600, p)
    assert 650 < len(exp[1]) < 760 and max(exp[2]) >= 2 and len(exp_many[1]) > 1400
    exp_joined = IB.concat([exp_many, exp, exp_many])

    def run(cap):
        R = pkg.index.ResidentIndex
        built = R.from_records(records, like, groups, 11)
        assert TIB.triple(built) == exp, cap
        lots = R.from_records(many, like)
        assert TIB.triple(lots) == exp_many, cap
        assert TIB.triple(R.concat([lots, built, lots])) == exp_joined, cap

    under_caps(pkg, grid, run, at_least=5)


# ---------------------------------------------------------------------------------- the constant grid limits, at their natural size

@pytest.fixture(scope="module")
def large(pkg):
    """a query of 70 000 hashes; node 0 holds all of them, three small nodes a few of them and a few others"""
    rng = np.random.default_rng(53)
    allh = np.unique(rng.integers(0, M64, 71_000, dtype=np.uint64))[:70_300]
    query, outside = [int(x) for x in allh[:70_000]], [int(x) for x in allh[70_000:]]
    sketches = [query, query[10:3000:7] + outside[:100], query[50_000::11] + outside[100:200], outside[200:]]
    ab = {h: 1 + h % 3 for h in query}
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    return sketches, query, ab, index, GR.gather(sketches, query, ab)


def test_gather_subtract_beyond_its_grid(pkg, large):
    """70 000 hits of the winner against the 256 workgroups x 256 hits of k_gather_subtract's grid: a second, part-filled trip"""
    sketches, query, ab, index, exp = large
    assert exp[0][0]["common_remaining"] == 70_000 > 256 * 256 and pkg.matrix.grid_cap() == 0
    res = index.gather(mk(pkg, query, ab), threshold_bp=1, scaled=1, abund_stats=False)
    assert TG.as_dicts(res.rows) == exp[0] and res.assigned.tolist() == exp[1]


def test_gather_many_subtract_beyond_its_grid(pkg, large):
    """... and against the 32 workgroups x 256 hits per query of k_gm_subtract's: 9 trips, with the query twice in the batch"""
    sketches, query, ab, index, exp = large
    assert exp[0][0]["common_remaining"] > 8 * 32 * 256 and pkg.matrix.grid_cap() == 0
    res = index.gather_many([mk(pkg, query, ab), mk(pkg, query, ab)], threshold_bp=1, scaled=1, abund_stats=False)
    for r in res:
        assert TGM.as_dicts(r.rows) == exp[0] and r.assigned.tolist() == exp[1]
