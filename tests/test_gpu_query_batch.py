"""How a batch of sketches reaches the device for gather_many, search_many and lca_counts (smh_index_gather_many,
smh_index_search_many, smh_index_lca_many): the same small index under every composition of the batch -- all queries on the
host, all resident in HBM, mixed, mixed with empty sketches first, in the middle and last -- and, for gather_many, every form
a query's abundances take, in one batch.  Every result must EQUAL the plain-Python restatement (all outputs are integers), no
call may bring a resident query to the host, and query_offsets are the cumulative sketch lengths.

The hashes of every node and query are match_restatement.window_hashes of the synthetic genome, not the library's: a query in
HBM is sketched from the same bases by the library, so a staging that misplaced a query would meet the restatement of another."""
import collections
import ctypes as C

import numpy as np
import pytest

import gather_restatement as GR
import lca_restatement as LR
import match_restatement as MR
import search_many_restatement as SR
import test_gpu_gather_many as TGM
import test_gpu_search_many as TS

pytestmark = pytest.mark.gpu

K, MX = 21, (1 << 64) // 20
NO = LR.NO_TAXON
PARENT = [0, 0, 0, 1, 1, 2, 3]
NODE_TAXON = [3, 4, 5, 6, NO, 1, 2, 3, 6, 5]
mk, count = TGM.mk, TGM.count
u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


class World:
    """ten nodes of 4 000 bases cut from a 30 000-base genome, and the hashes of any of its segments"""

    def __init__(self, pkg, pyoracle):
        self.pkg = pkg
        self.genome = pyoracle.synth_dna(0, 30000, 21)
        self.window = MR.window_hashes(self.genome, K)            # window p -> its hash
        assert len(self.window) == 30000 - K + 1
        self.nodes = [sorted(self.sketch_of([[(a, min(a + 4000, 30000))]])) for a in range(0, 30000, 3000)]
        assert len(self.nodes) == 10 and all(100 < len(n) < 400 for n in self.nodes)
        self.owners = LR.owners_of(self.nodes)
        self.index = pkg.index.ResidentIndex([mk(pkg, n, max_hash=MX) for n in self.nodes])
        self.index.set_taxonomy(PARENT, NODE_TAXON)
        self.expected = {}
        self.blank = next(p for p in range(len(self.window)) if self.window[p] > MX)   # a window that leaves nothing in a sketch

    def sketch_of(self, batches):
        """{hash: abundance} of the records [a, b) of every batch"""
        c = collections.Counter()
        for batch in batches:
            for a, b in batch:
                c.update(h for h in self.window[a:b - K + 1] if h <= MX)
        return dict(c)


class Query:
    """a query to be: `batches` of records of the genome, where it lives and whether it tracks abundances.  hashes / abunds:
    what it holds by the restatement (abunds None: it does not track).  A host query that tracks carries 1 + h % 5 instead of
    its counts, so that a weight taken from a neighbour shows."""

    def __init__(self, world, batches, hbm, track, blank=False):
        self.w, self.batches, self.hbm, self.track, self.blank = world, batches, hbm, track, blank
        held = world.sketch_of(batches)
        self.hashes = sorted(held)
        self.abunds = None if not track else held if hbm else {h: 1 + h % 5 for h in held}
        self.key = (repr(batches), None if not track else "counts" if hbm else "1 + h % 5")   # what the restatement sees

    def make(self):
        pkg, w = self.w.pkg, self.w
        if not self.hbm:
            return mk(pkg, self.hashes, self.abunds, max_hash=MX, track=self.track)
        mh = pkg.KmerMinHash(0, K, False, 42, MX, self.track)
        for batch in self.batches:                               # one device pass per batch: run starts, then u64 counts
            mh.add_sequences([w.genome[a:b] for a, b in batch], True)
        if self.blank:                                           # sketched on the device, and nothing was kept
            mh.add_sequences([w.genome[w.blank:w.blank + K]], True)
        assert len(mh) == len(self.hashes)
        return mh


@pytest.fixture(scope="module")
def world(pkg, pyoracle):
    return World(pkg, pyoracle)


ONE = ([[(0, 9000)]], [[(5000, 12000)]], [[(10000, 16000), (11000, 14000)]], [[(15000, 22000)], [(18000, 25000)]], [[(21000, 30000)]])


def compose(world, name):
    q = lambda k, hbm, track=False: Query(world, ONE[k], hbm, track)
    empty = lambda hbm, track=False: Query(world, [], hbm, track, blank=True)
    if name == "host":
        return [q(0, False), q(1, False, True), q(2, False), q(3, False, True), q(4, False)]
    if name == "hbm":
        return [q(0, True), q(1, True, True), q(2, True, True), q(3, True, True), q(4, True)]
    if name == "mixed":
        return [q(0, True), q(1, False), q(2, True, True), q(3, False, True), q(4, True), q(3, True, True)]
    if name == "mixed_empty_host":
        return [empty(False), q(0, True), q(1, False), empty(False, True), q(2, True, True), q(3, False, True), empty(False)]
    if name == "mixed_empty_hbm":
        return [empty(True), q(0, True), q(1, False), empty(True, True), q(3, True, True), q(2, False, True), empty(True)]
    if name == "abundance_forms":
        # host tracking, host not tracking (weights 1), HBM of one pass (run starts), HBM of two passes (u64 counts), HBM not tracking
        return [q(1, False, True), q(0, False), q(2, True, True), q(3, True, True), q(4, True)]
    if name == "hbm_none_tracks":
        return [q(0, True), q(2, True), q(3, True)]
    raise KeyError(name)


COMPOSITIONS = ("host", "hbm", "mixed", "mixed_empty_host", "mixed_empty_hbm")


def expected(world, op, q):
    """the restatement's answer for one query, computed once per (operation, query content)"""
    key = (op,) + q.key
    if key not in world.expected:
        if op == "gather_many":
            world.expected[key] = GR.gather(world.nodes, q.hashes, q.abunds, 1)
        elif op == "search_many":
            world.expected[key] = SR.search_many(world.nodes, [q.hashes], SR.JACCARD, 0.02, 0)[0]
        else:
            world.expected[key] = LR.counts(PARENT, NODE_TAXON, world.owners, q.hashes)
    return world.expected[key]


def query_offsets_of(pkg, index, op, sketches):
    """query_offsets as the C call writes them (the Python methods use them and do not hand them on)"""
    L = pkg.lib()
    n = len(sketches)
    arr = (C.c_void_p * max(n, 1))(*[s._p for s in sketches])
    off, q_off = np.zeros(n + 1, dtype=np.uint64), np.full(n + 1, TGM.SENTINEL, dtype=np.uint64)
    L.sourmash_err_clear()
    if op == "gather_many":
        rows_p = C.POINTER(pkg._lib.SmhGatherRow)()
        rc = L.smh_index_gather_many(index._h, arr, n, 1, 1000, off.ctypes.data_as(u64p), C.byref(rows_p), q_off.ctypes.data_as(u64p), None)
        outs = [rows_p]
    else:
        tp, cp = u32p(), u64p()
        rc = L.smh_index_lca_many(index._h, arr, n, off.ctypes.data_as(u64p), C.byref(tp), C.byref(cp), q_off.ctypes.data_as(u64p), None)
        outs = [tp, cp]
    assert rc == 0
    for p in outs:
        pkg.minhash._free(C.cast(p, C.c_void_p))
    return q_off.tolist()


def run(world, op, queries):
    pkg, index = world.pkg, world.index
    sketches = [q.make() for q in queries]
    before = count(pkg, "sketch_to_host")
    if op == "gather_many":
        res = index.gather_many(sketches, threshold_bp=1, scaled=1, abund_stats=False)
        got = [(TGM.as_dicts(r.rows), r.assigned.tolist()) for r in res]
    elif op == "search_many":
        got = TS.per_query(index.search_many(sketches, 0.02, "jaccard", threshold_bp=0, scaled=1))
    else:
        got = [(list(zip(t.tolist(), c.tolist())), per.tolist()) for t, c, per in index.lca_counts(sketches, hash_taxon=True)]
    if op != "search_many":
        lens = np.cumsum([0] + [len(q.hashes) for q in queries]).tolist()
        assert query_offsets_of(pkg, index, op, sketches) == lens
    assert count(pkg, "sketch_to_host") == before, "%s brought a device-resident query to the host" % op
    assert len(got) == len(queries)
    for k, q in enumerate(queries):
        assert got[k] == expected(world, op, q), (op, k)
    resident = [s for s, q in zip(sketches, queries) if q.hbm and not q.blank]
    for s in resident:                                           # they were resident: looking at one moves it now
        s.mins
    assert count(pkg, "sketch_to_host") == before + len(resident)
    return got


@pytest.mark.parametrize("composition", COMPOSITIONS)
@pytest.mark.parametrize("op", ["gather_many", "search_many", "lca_counts"])
def test_batch_compositions(world, op, composition):
    queries = compose(world, composition)
    assert all(200 < len(q.hashes) < 700 or q.blank for q in queries)
    got = run(world, op, queries)
    full = [g for g, q in zip(got, queries) if not q.blank]
    if op == "gather_many":
        assert all(len(rows) >= 2 and GR.UNASSIGNED not in assigned for rows, assigned in full)
        assert all(g == ([], []) for g, q in zip(got, queries) if q.blank)
    elif op == "search_many":
        assert all(2 <= len(rows) < 10 for rows in full)          # the threshold selects among the nodes that share a hash
        assert all(g == [] for g, q in zip(got, queries) if q.blank)
    else:
        assert all(len(pairs) >= 2 and len(per) == len(q.hashes) for (pairs, per), q in zip(got, queries) if not q.blank)
        assert all(g == ([], []) for g, q in zip(got, queries) if q.blank)


@pytest.mark.parametrize("composition", ["abundance_forms", "hbm_none_tracks"])
def test_gather_many_abundance_forms(world, composition):
    queries = compose(world, composition)
    got = run(world, "gather_many", queries)
    for (rows, _), q in zip(got, queries):
        weighted = any(r["abund_sum"] != r["common_remaining"] for r in rows)
        assert weighted == (q.abunds is not None), "a query's weights are its own"
    if composition == "abundance_forms":
        runs, counts = queries[2].abunds, queries[3].abunds
        assert set(runs.values()) == {1, 2} and set(counts.values()) == {1, 2}
