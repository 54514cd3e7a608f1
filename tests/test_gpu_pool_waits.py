"""Who waits for the whole device when a block goes back to the pool, and what a refusal leaves behind.  The index operations
borrow their device work space through a Workspace (csrc/device.hpp): it waits for the call's own stream and gives its blocks
back without hipDeviceSynchronize().  Every block that does go back behind the device-wide wait is counted as
"pool_free_waited", so on a success path of an index operation that counter stands still.  One tiny scaled index serves every
case: 8 nodes of about 50 hashes with abundances under a three-level taxonomy, 3 queries, 4 records; the budgets of the
batched calls are set so low that each takes two chunks at least (asserted on the *_chunk counters).  What the calls return
is checked against the restatements and the oracle in the other files; here only the waits count, and that the library
answers as before after a call was refused half way.

A sketch or an index that dies gives its own buffers back behind the device-wide wait, by design: everything a case makes
stays referenced until the counter has been read."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
WAITED = "pool_free_waited"
K = 21


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


def sketch_of(pkg, seq, twice=False):
    mh = pkg.KmerMinHash(0, K, False, 42, M64, True)
    mh.add_sequence(seq, True)
    if twice:
        mh.add_sequence(seq[:40], True)                           # abundances of 2 on the first k-mers
    return mh


class Tiny:
    """the sequences and sketches of every case; the indexes are made anew per case (make_index), so that the structures an
    index builds on first use -- the hash directory, the LCA table, the abundances in HBM -- are built inside the measured call"""

    def __init__(self, pkg):
        rng = np.random.default_rng(5)
        genome = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=160))
        self.seqs = [genome[9 * v:9 * v + 70] for v in range(8)]   # 50 k-mers each, neighbours share 41
        self.nodes = [sketch_of(pkg, s, v % 2 == 1) for v, s in enumerate(self.seqs)]
        self.queries = [sketch_of(pkg, genome[a:a + 70]) for a in (4, 31, 77)]
        self.records = [genome[0:60], genome[50:75], genome[100:160], genome[20:30]]   # the last one has no window
        self.parent = [0, 0, 0, 1, 1, 2]                           # root; two children; three grandchildren
        self.node_taxon = [3, 3, 4, 4, 5, 5, 1, 2]
        self.like = pkg.KmerMinHash(0, K, False, 42, M64, True)
        assert all(45 <= len(mh.mins) <= 50 for mh in self.nodes + self.queries)

    def make_index(self, pkg, taxonomy=False):
        index = pkg.index.ResidentIndex(self.nodes)
        if taxonomy:
            index.set_taxonomy(self.parent, self.node_taxon)
        return index


@pytest.fixture(scope="module")
def tiny(pkg):
    return Tiny(pkg)


@pytest.fixture
def low_budgets(pkg):
    """one query per chunk: 8 (query, node) counters for 8 nodes, 60 keys for queries of about 50 hashes"""
    m = pkg.matrix
    try:
        m.set_search_many_budget(8); m.set_gather_many_budget(8); m.set_lca_budget(60)
        yield
    finally:
        m.set_search_many_budget(0); m.set_gather_many_budget(0); m.set_lca_budget(0)


def quiet(pkg, what, fn, chunks=None, at_least=2):
    """fn() without a device-wide wait; chunks: the counter that must rise by at_least.  Returns what fn made -- the caller
    keeps it, so nothing of it dies before the counter is read."""
    before, chunks_before = count(pkg, WAITED), count(pkg, chunks) if chunks else 0
    out = fn()
    moved = count(pkg, WAITED) - before
    ran = count(pkg, chunks) - chunks_before if chunks else None
    print("%s: %s moved by %d%s" % (what, WAITED, moved, "" if chunks is None else ", %s by %d" % (chunks, ran)))
    assert moved == 0, (what, moved)
    assert chunks is None or ran >= at_least, (what, chunks, ran)
    return out


def test_the_counter_counts(pkg, tiny):
    """an index that dies gives its arrays back behind the device-wide wait: the counter the other cases read is alive"""
    index = tiny.make_index(pkg)
    before = count(pkg, WAITED)
    del index
    gc.collect()
    assert count(pkg, WAITED) >= before + 3                       # hashes, offsets, nums at least


def test_search_and_nearest(pkg, tiny, low_budgets):
    index = tiny.make_index(pkg)
    kept = [quiet(pkg, "search_many", lambda: index.search_many(tiny.queries, 0.0, "jaccard", scaled=1), "search_many_chunk"),
            quiet(pkg, "search_self", lambda: index.pairwise(0.0, "jaccard", upper=False), "search_many_chunk"),
            quiet(pkg, "nearest_many", lambda: index.nearest(tiny.queries, 2, "jaccard", scaled=1), "nearest_chunk"),
            quiet(pkg, "nearest_self", lambda: index.knn(2, "jaccard"), "nearest_chunk")]
    assert all(len(r) > 0 for r in kept)
    assert len(kept[2]) == 2 * len(tiny.queries) and len(kept[3]) == 2 * len(tiny.nodes)


def test_gather_gather_many_and_lca_many(pkg, tiny, low_budgets):
    index = tiny.make_index(pkg, taxonomy=True)
    one = quiet(pkg, "gather", lambda: index.gather(tiny.queries[0], threshold_bp=1, scaled=1, abund_stats=False))
    many = quiet(pkg, "gather_many", lambda: index.gather_many(tiny.queries, threshold_bp=1, scaled=1, abund_stats=False), "gather_many_chunk")
    counts = quiet(pkg, "lca_many", lambda: index.lca_counts(tiny.queries, hash_taxon=True), "lca_chunk")
    assert len(one.rows) > 0 and len(many) == len(counts) == len(tiny.queries) and all(len(r.rows) > 0 for r in many)
    assert all(int(cnt.sum()) > 0 for _, cnt, _ in counts)


def test_match_and_lca_on_records(pkg, tiny):
    index = tiny.make_index(pkg, taxonomy=True)
    hits = quiet(pkg, "match with hits", lambda: index.match(tiny.records, hits=True))
    plain = quiet(pkg, "match", lambda: index.match(tiny.records))
    rows = quiet(pkg, "lca on records", lambda: index.lca_classify_records(tiny.records))
    assert hits.hit_distinct.tolist() == plain.hit_distinct.tolist() == rows.hit_distinct.tolist()
    assert hits.hit_distinct[0] > 0 and hits.windows.tolist() == [40, 5, 40, 0] and len(hits.hit_hashes) == int(hits.hit_distinct.sum())


@pytest.mark.parametrize("linkage", ["components", "greedy"])
def test_cluster(pkg, tiny, low_budgets, linkage):
    index = tiny.make_index(pkg)
    got = quiet(pkg, "cluster, " + linkage, lambda: index.cluster(0.0, "jaccard", linkage, scaled=1), "cluster_chunk")
    assert 1 <= got.n_clusters < len(tiny.nodes)


def test_children_of_an_index(pkg, tiny):
    index = tiny.make_index(pkg, taxonomy=True)
    kept = [quiet(pkg, "collapse", lambda: index.collapse([0, 0, 1, 1, 2, 2, 0, 1], 3, abund="sum")),
            quiet(pkg, "filter", lambda: index.filter(tiny.queries[1], "keep", abund="operand")),
            quiet(pkg, "filter, owners", lambda: index.filter(min_owners=2)),
            quiet(pkg, "select", lambda: index.select([7, 2, 2, 0])),
            quiet(pkg, "downsample", lambda: index.downsample(max_hash=M64 // 2))]
    assert [len(c) for c in kept] == [3, 8, 8, 4, 8]
    assert all(int(c.read()[0][-1]) > 0 for c in kept)


def test_angular(pkg, tiny):
    rows, cols = tiny.make_index(pkg), tiny.make_index(pkg)
    kept = [quiet(pkg, "angular, index vs index", lambda: rows.angular_matrix(cols)),
            quiet(pkg, "angular, index vs itself", lambda: rows.angular_matrix()),
            quiet(pkg, "angular, query vs index", lambda: cols.angular(tiny.queries[2]))]
    assert kept[2].dot.shape == (len(tiny.nodes),) and int(kept[2].dot.sum()) > 0


def test_index_build_and_concat(pkg, tiny):
    R = pkg.index.ResidentIndex
    built = quiet(pkg, "index build", lambda: R.from_records(tiny.records, tiny.like))
    grouped = quiet(pkg, "index build, groups", lambda: R.from_records(tiny.records, tiny.like, [1, 0, 1, 0], 2))
    joined = quiet(pkg, "concat", lambda: R.concat([built, grouped, built]))
    sizes = built.sizes().tolist()
    assert len(sizes) == 4 and min(sizes[:3]) > 0 and sizes[3] == 0 and len(grouped) == 2 and len(joined) == 10


def test_a_refusal_leaves_the_library_usable(pkg, tiny, low_budgets):
    """the greedy linkage under a pair budget of 1 is refused after its first chunks have run, with their kernels queued and
    their blocks held: the blocks go back behind a wait for the stream, and the same index answers search_self as before"""
    index = tiny.make_index(pkg)
    rows_of = lambda res: (res.offsets.tolist(), res.node.tolist(), res.common.tolist(), res.node_size.tolist(), res.query_size.tolist())
    before = rows_of(index.pairwise(0.0, "jaccard", upper=False))
    assert len(before[1]) > 1
    waited = count(pkg, WAITED)
    try:
        pkg.matrix.set_cluster_pair_budget(1)
        with pytest.raises(pkg.SourmashError) as ei:
            index.cluster(0.0, "jaccard", "greedy", scaled=1)
    finally:
        pkg.matrix.set_cluster_pair_budget(0)
    assert ei.value.code == 3 and ei.value.message.startswith("cluster: the greedy linkage holds the directed adjacency in device memory")
    assert "the pair budget is 1 " in ei.value.message
    assert count(pkg, WAITED) == waited                           # the refusal waits for its stream, not for the device
    assert rows_of(index.pairwise(0.0, "jaccard", upper=False)) == before
    assert index.cluster(0.0, "jaccard", "greedy", scaled=1).n_clusters >= 1
