"""Gather of a batch of queries on the device (smh_index_gather_many, smh_index_gather_block_dev,
ResidentIndex.gather_many) against the plain-Python restatement run per query: rows and `assigned` must be EQUAL -- every
output is an integer.  ResidentIndex.gather is the second witness where the derived floats matter."""
import ctypes as C

import numpy as np
import pytest

import gather_restatement as GR

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
FIELDS = ("match", "common_remaining", "common_original", "size_match", "abund_sum")
SENTINEL = 0xDEADBEEFDEADBEEF


def mk(pkg, hashes, abunds=None, max_hash=M64, track=False, ksize=21, seed=42, protein=False, num=0):
    """a sketch holding `hashes`; abunds ({hash: abundance}) makes it track abundances"""
    mh = pkg.KmerMinHash(num, ksize, protein, seed, max_hash, track or abunds is not None)
    h = sorted(int(x) for x in hashes)
    if abunds is not None and h:
        mh.add_many_with_abund([(x, abunds[x]) for x in h])
    elif h:
        mh.add_many(np.array(h, dtype=np.uint64))
    return mh


def as_dicts(rows):
    return [{f: getattr(r, f) for f in FIELDS} for r in rows]


def run_many(index, queries, threshold=0, capacity=None):
    """[(rows as dicts, assigned as list)] with threshold_common and the capacity handed over as they are (scaled = 1)"""
    res = index.gather_many(queries, threshold_bp=threshold, scaled=1, max_rows=capacity)
    assert len(res) == len(queries)
    return [(as_dicts(r.rows), r.assigned.tolist()) for r in res]


def check_many(pkg, sketches, queries, abunds=None, threshold=0, capacity=None, index=None):
    """queries: lists of hashes; abunds: one {hash: abundance} (or None) per query"""
    index = index or pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    abunds = abunds or [None] * len(queries)
    got = run_many(index, [mk(pkg, q, a) for q, a in zip(queries, abunds)], threshold, capacity)
    for k, (q, a) in enumerate(zip(queries, abunds)):
        exp = GR.gather(sketches, q, a, threshold, capacity)
        assert got[k][0] == exp[0], k
        assert got[k][1] == exp[1], k
    return got


def same(a, b):
    """two GatherResults, field for field (the derived floats included)"""
    return list(a.rows) == list(b.rows) and a.assigned.dtype == b.assigned.dtype and np.array_equal(a.assigned, b.assigned)


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


# ---------------------------------------------------------------------------------- 1, 9: the committed fixture

class Fixture:
    def __init__(self, pkg, sketches):
        self.mins = [s["mins"] for s in sketches]
        self.max_hash = sketches[0]["max_hash"]
        self.abs = [dict(zip(s["mins"], s["abundances"])) for s in sketches]
        union = {}
        for ab in self.abs:
            for h, a in ab.items():
                union[h] = union.get(h, 0) + a
        foreign = [h + 1 for h in sorted(union)[:300] if h + 1 not in union]
        # the union, every single sketch, an empty query, foreign hashes only, the union again
        self.q_hashes = [sorted(union)] + self.mins + [[], foreign, sorted(union)]
        self.q_abunds = [union] + self.abs + [{}, {h: 3 for h in foreign}, union]
        nodes = [mk(pkg, m, ab, max_hash=self.max_hash) for m, ab in zip(self.mins, self.abs)]
        self.index = pkg.index.ResidentIndex(nodes)
        self.queries = {True: [mk(pkg, q, a, max_hash=self.max_hash) for q, a in zip(self.q_hashes, self.q_abunds)],
                        False: [mk(pkg, q, max_hash=self.max_hash) for q in self.q_hashes]}
        self._exp = {}

    def expected(self, with_abund, threshold, capacity=None):
        """one full restatement run per query and (abundances, threshold); a capacity cuts it (gather_restatement.cut)"""
        key = (with_abund, threshold)
        if key not in self._exp:
            runs = [GR.gather(self.mins, q, a if with_abund else None, threshold) for q, a in zip(self.q_hashes[:-1], self.q_abunds)]
            self._exp[key] = runs + [runs[0]]
        return [(r, a) if capacity is None else GR.cut(r, a, capacity) for r, a in self._exp[key]]


@pytest.fixture(scope="module")
def fx(pkg, sbt_subset_sketches):
    return Fixture(pkg, sbt_subset_sketches)


@pytest.mark.parametrize("with_abund", [True, False])
@pytest.mark.parametrize("threshold", [1, 50])
def test_fixture_batch(fx, with_abund, threshold):
    for cap in (None, 0, 1, 7):
        got = run_many(fx.index, fx.queries[with_abund], threshold, cap)
        exp = fx.expected(with_abund, threshold, cap)
        for k in range(len(exp)):
            assert got[k][0] == exp[k][0], (cap, k)
            assert got[k][1] == exp[k][1], (cap, k)
        assert got[0] == got[-1]
    full = fx.expected(with_abund, threshold)
    assert len(full[0][0]) == (99 if threshold == 1 else 82) and full[101] == ([], []) and full[102][0] == []
    if with_abund:
        assert any(r["abund_sum"] != r["common_remaining"] for r in full[0][0])


@pytest.mark.parametrize("with_abund", [True, False])
def test_fixture_derived_values(fx, with_abund):
    """field for field what ResidentIndex.gather gives, the floats included; threshold_bp goes through scaled"""
    qs = fx.queries[with_abund]
    for kw in (dict(threshold_bp=99_500), dict(threshold_bp=0, max_rows=3), dict(threshold_bp=99_500, abund_stats=False)):
        many = fx.index.gather_many(qs, **kw)
        for k in (0, 1, 2, 50, 100, 101, 102, 103):
            assert same(many[k], fx.index.gather(qs[k], **kw)), (kw, k)
    rows = fx.expected(with_abund, 50)
    many = fx.index.gather_many(qs, threshold_bp=99_500)
    assert [as_dicts(m.rows) for m in many] == [r for r, _ in rows]


@pytest.mark.parametrize("with_abund", [True, False])
def test_csr_device_form(pkg, fx, with_abund):
    import torch
    L = pkg.lib()
    flat, off = pkg.matrix.csr_from_sketches([np.array(q, dtype=np.uint64) for q in fx.q_hashes])
    ab = np.array([a[h] for q, a in zip(fx.q_hashes, fx.q_abunds) for h in q], dtype=np.uint64)
    t_h = torch.from_numpy(flat.view(np.int64)).cuda()
    t_a = torch.from_numpy(ab.view(np.int64)).cuda()
    u64p = C.POINTER(C.c_uint64)

    def call(index, cap):
        row_off = np.full(len(off), SENTINEL, dtype=np.uint64)
        assigned = np.zeros(flat.size, dtype=np.uint32)
        rows_p = C.POINTER(pkg._lib.SmhGatherRow)()
        L.sourmash_err_clear()
        torch.cuda.synchronize()
        rc = L.smh_index_gather_block_dev(index._h, C.c_void_p(t_h.data_ptr()), C.c_void_p(t_a.data_ptr() if with_abund else 0),
                                          off.ctypes.data_as(u64p), len(off) - 1, 50, cap, row_off.ctypes.data_as(u64p),
                                          C.byref(rows_p), assigned.ctypes.data_as(C.POINTER(C.c_uint32)), None)
        if rc:
            L.sourmash_err_clear()
            return rc, row_off, None
        out = []
        for k in range(len(off) - 1):
            rows = [{f: getattr(rows_p[r], f) for f in FIELDS} for r in range(int(row_off[k]), int(row_off[k + 1]))]
            out.append((rows, assigned[int(off[k]):int(off[k + 1])].tolist()))
        pkg.minhash._free(C.cast(rows_p, C.c_void_p))
        return 0, row_off, out

    for cap in (1000, 7):
        rc, _, got = call(fx.index, cap)
        assert rc == 0
        exp = fx.expected(with_abund, 50, cap)
        assert got == [(r, a) for r, a in exp]
    odd = pkg.index.ResidentIndex([mk(pkg, fx.mins[0], max_hash=fx.max_hash), mk(pkg, fx.mins[1], max_hash=fx.max_hash, seed=43)])
    rc, row_off, _ = call(odd, 10)
    assert rc == 3 and (row_off == SENTINEL).all()


# ---------------------------------------------------------------------------------- 2: the directory search

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
    got = check_many(pkg, sketches, queries)
    assert sum(r["common_remaining"] for r in got[0][0]) == 2 and got[0][1] != [GR.UNASSIGNED] * 2   # both ends were found
    assert got[2][0] == [] and len(got[1][0]) >= 2
    assert GR.UNASSIGNED not in got[1][1] and GR.UNASSIGNED not in got[4][1]


# ---------------------------------------------------------------------------------- 3: owner lists

def test_owner_list_edges(pkg):
    """hashes held by 1, 8, 9, 64, 65 and 3 010 nodes in one query (lists walked by a lane and by the wave); the first
    nodes also hold private hashes, 20 - i of them, which forces some rounds"""
    n = 3010
    shared = {k: (1 << 60) + k for k in (1, 8, 9, 64, 65, n)}
    sketches, nxt = [], 1
    for i in range(n):
        s = [h for k, h in shared.items() if i < k] + list(range(nxt, nxt + max(0, 20 - i)))
        nxt += max(0, 20 - i)
        sketches.append(s)
    everything = sorted(set().union(*sketches))
    got = check_many(pkg, sketches, [everything, [shared[n]], sorted(shared.values())])
    assert [r["match"] for r in got[0][0]] == list(range(20))
    assert got[1][0] == [dict(match=0, common_remaining=1, common_original=1, size_match=26, abund_sum=1)]
    assert len(got[2][0]) == 1 and got[2][0][0]["common_remaining"] == 6


# ---------------------------------------------------------------------------------- 4: rounds

def test_queries_ending_in_different_rounds(pkg):
    B = pkg.lib().smh_gather_rounds_per_sync()
    want = [0, 1, B - 1, B, B + 1, 2 * B + 6]
    rng = np.random.default_rng(3)
    sketches, queries, nxt = [], [], 10
    for rounds in want:   # a chain of disjoint sketches of sizes rounds .. 1: exactly `rounds` rounds
        q = []
        for size in range(rounds, 0, -1):
            sketches.append(list(range(nxt, nxt + size)))
            q += sketches[-1]
            nxt += size
        queries.append(q if rounds else [5, 6, 7])
    order = [int(i) for i in rng.permutation(len(sketches))]
    sketches = [sketches[i] for i in order]
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    got = check_many(pkg, sketches, queries, index=index)
    assert [len(g[0]) for g in got] == want
    back = check_many(pkg, sketches, queries[::-1], index=index)
    assert back == got[::-1]
    capped = check_many(pkg, sketches, queries, capacity=B, index=index)
    assert [len(g[0]) for g in capped] == [min(w, B) for w in want]


# ---------------------------------------------------------------------------------- 5: chunks

def test_chunking_changes_no_result(pkg):
    rng = np.random.default_rng(14)
    n, nq = 50, 9
    universe = [int(x) for x in rng.integers(0, M64, 2000, dtype=np.uint64)]
    sketches = [[int(x) for x in rng.choice(universe, 120, replace=False)] for _ in range(n)]
    queries = [[int(x) for x in rng.choice(universe, 100 + 50 * k, replace=False)] for k in range(nq)]
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    default = pkg.matrix.gather_many_budget()
    assert default == 1 << 26
    base = check_many(pkg, sketches, queries, threshold=2, index=index)
    qs = [mk(pkg, q) for q in queries]
    try:
        for budget in (1, 50, 51, 100, 449, 450, 0):
            pkg.matrix.set_gather_many_budget(budget)
            eff = budget or default
            assert pkg.matrix.gather_many_budget() == eff
            per = min(max(eff // n, 1), 65535)           # the cutter's rule: as many queries as the budget holds counters for
            before = count(pkg, "gather_many_chunk")
            assert run_many(index, qs, 2) == base, budget
            assert count(pkg, "gather_many_chunk") - before == -(-nq // per), budget
    finally:
        pkg.matrix.set_gather_many_budget(0)
    assert [-(-nq // min(max(b // n, 1), 65535)) for b in (1, 50, 51, 100, 449, 450, default)] == [9, 9, 9, 5, 2, 1, 1]


# ---------------------------------------------------------------------------------- 6: isolation

def test_the_same_large_query_four_times(pkg):
    """40 000 hashes = 320 KB, larger than any LDS sample, four times among four other queries"""
    rng = np.random.default_rng(5)
    allh = np.unique(rng.integers(0, M64, 90_000, dtype=np.uint64))
    query = allh[:40_000 * 2:2][:40_000]
    outside = np.setdiff1d(allh, query)
    sketches = []
    for i in range(300):
        la = int(rng.integers(50, 501))
        k = int(rng.integers(0, la + 1)) if i % 7 else la
        sketches.append(np.concatenate([rng.choice(query, k, replace=False), rng.choice(outside, la - k, replace=False)]))
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    ab = {int(h): int(a) for h, a in zip(query, rng.integers(1, 1000, query.size))}
    big = mk(pkg, query, ab)
    others = [mk(pkg, rng.choice(allh, 3000 * (k + 1), replace=False)) for k in range(4)]
    batch = [big, others[0], big, others[1], others[2], big, others[3], big]
    res = index.gather_many(batch, threshold_bp=3, scaled=1)
    single = index.gather(big, threshold_bp=3, scaled=1)
    assert len(single.rows) > 100
    for k in (0, 2, 5, 7):
        assert same(res[k], single), k
    for k, o in zip((1, 3, 4, 6), others):
        assert same(res[k], index.gather(o, threshold_bp=3, scaled=1)), k


# ---------------------------------------------------------------------------------- 7: ties

def test_tie_rule_across_the_batch(pkg):
    sketches = [[1, 2, 3], [4, 5, 6], [1, 2, 3], [10, 11], [12, 13], [10, 11], [20]]
    queries = [[1, 2, 3, 4, 5, 6], [10, 11, 12, 13], [12, 13, 1, 2, 20]]
    got = check_many(pkg, sketches, queries)
    assert [r["match"] for r in got[0][0]] == [0, 1] and GR.ties(sketches, queries[0]) == [0]
    assert [r["match"] for r in got[1][0]] == [3, 4] and GR.ties(sketches, queries[1]) == [0]
    assert [r["match"] for r in got[2][0]] == [0, 4, 6] and GR.ties(sketches, queries[2]) == [0]


# ---------------------------------------------------------------------------------- 8: queries in HBM

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
        twins = [sketched(p, track) for p in parts]
        hosts = [mk(pkg, t.mins, dict(zip(t.mins, t.abunds)) if track else None, max_hash=mx) for t in twins]
        resident = [sketched(p, track) for p in parts]
        batch = [resident[0], hosts[1], resident[2], resident[3]]          # HBM and host states in one batch
        before = count(pkg, "sketch_to_host")
        res = index.gather_many(batch, threshold_bp=1, scaled=1, abund_stats=False)
        assert count(pkg, "sketch_to_host") == before, "gather_many brought a device-resident query to the host"
        ref = index.gather_many(hosts, threshold_bp=1, scaled=1, abund_stats=False)
        for k in range(4):
            assert same(res[k], ref[k]), (track, k)
            exp = GR.gather(node_mins, hosts[k].mins, dict(zip(hosts[k].mins, hosts[k].abunds)) if track else None, 1)
            assert (as_dicts(res[k].rows), res[k].assigned.tolist()) == exp and len(exp[0]) >= 3
        # they were resident: looking at one moves it now
        assert resident[0].mins == hosts[0].mins
        assert count(pkg, "sketch_to_host") == before + 1


# ---------------------------------------------------------------------------------- 10: one directory for match and gather_many

def test_shared_directory(pkg, pyoracle):
    L = pkg.lib()
    genome = pyoracle.synth_dna(0, 3000, 4)
    records = [genome[:200], genome[200:500]]

    def fresh():
        probe = pkg.KmerMinHash(0, 21, False, 42, M64, False)
        probe.add_sequence(genome[:1000], True)
        ws = probe.mins
        return pkg.index.ResidentIndex([mk(pkg, ws[::2]), mk(pkg, ws[1::2]), mk(pkg, ws[::5])]), [mk(pkg, ws[::3]), mk(pkg, ws[:300])]

    index, qs = fresh()
    built = count(pkg, "match_directory_built")
    index.match(records)
    rows = run_many(index, qs)
    assert count(pkg, "match_directory_built") == built + 1
    other, qs2 = fresh()
    assert run_many(other, qs2) == rows and len(rows[0][0]) >= 2
    matched = other.match(records)
    assert count(pkg, "match_directory_built") == built + 2
    assert matched.best.tolist() == index.match(records).best.tolist()
    assert L.smh_release_workspace() == 0
    assert run_many(index, qs) == rows
    assert count(pkg, "match_directory_built") == built + 3
    run_many(index, qs)
    assert count(pkg, "match_directory_built") == built + 3


# ---------------------------------------------------------------------------------- 11: errors

def test_errors_write_nothing(pkg):
    L = pkg.lib()
    u64p = C.POINTER(C.c_uint64)
    nodes = [mk(pkg, [1, 2, 3]), mk(pkg, [3, 4])]
    index = pkg.index.ResidentIndex(nodes)
    good = [mk(pkg, [1, 2, 3, 4]) for _ in range(5)]
    assert [len(r[0]) for r in run_many(index, good)] == [2] * 5

    def raw(idx, queries, null_rows=False):
        arr = (C.c_void_p * len(queries))(*[q._p for q in queries])
        row_off = np.full(len(queries) + 1, SENTINEL, dtype=np.uint64)
        q_off = np.full(len(queries) + 1, SENTINEL, dtype=np.uint64)
        rows_p = C.POINTER(pkg._lib.SmhGatherRow)()
        L.sourmash_err_clear()
        rc = L.smh_index_gather_many(idx._h, arr, len(queries), 1, 10, row_off.ctypes.data_as(u64p), None if null_rows else C.byref(rows_p),
                                     q_off.ctypes.data_as(u64p), None)
        assert rc != 0 and not rows_p
        assert (row_off == SENTINEL).all() and (q_off == SENTINEL).all()
        with pytest.raises(pkg.SourmashError) as ei:
            pkg.errors.check()
        assert ei.value.code == rc
        return ei.value

    e = raw(index, good[:3] + [mk(pkg, [1, 2], num=5)] + good[4:])
    assert e.code == 3 and "query 3" in e.message and "scaled" in e.message
    e = raw(index, [good[0], mk(pkg, [1, 2], ksize=31), good[2], good[3], mk(pkg, [1, 2], seed=43)])
    assert e.code == 101 and "query 1" in e.message
    mixed = pkg.index.ResidentIndex(nodes + [mk(pkg, [1, 2, 9], num=5)])
    e = raw(mixed, good)
    assert e.code == 3 and "query 0" in e.message and "num sketch" in e.message
    raw(index, good, null_rows=True)
    with pytest.raises(pkg.SourmashError) as ei:
        index.gather_many(good[:2] + [mk(pkg, [1], max_hash=1 << 62)])
    assert ei.value.code == 103 and "query 2" in ei.value.message
    # zero rows and no error
    assert index.gather_many([]) == []
    assert run_many(pkg.index.ResidentIndex([]), [mk(pkg, [1, 2]), mk(pkg, [])]) == [([], [GR.UNASSIGNED] * 2), ([], [])]
    assert run_many(index, [mk(pkg, []), mk(pkg, [10, 11])]) == [([], []), ([], [GR.UNASSIGNED] * 2)]
    assert run_many(pkg.index.ResidentIndex([mk(pkg, []), mk(pkg, [])]), [mk(pkg, [1])]) == [([], [GR.UNASSIGNED])]
    assert run_many(index, good, threshold=4) == [([], [GR.UNASSIGNED] * 4)] * 5


# ---------------------------------------------------------------------------------- 12: downsample

def test_downsample_groups(pkg):
    rng = np.random.default_rng(12)
    top = 1 << 60
    pool = np.unique(rng.integers(1, top, 4000, dtype=np.uint64))
    at = top // 4                                                          # the index's own resolution
    nodes = [mk(pkg, [int(h) for h in rng.choice(pool, 600, replace=False) if h <= at], max_hash=at) for _ in range(12)]
    index = pkg.index.ResidentIndex(nodes)
    queries = []
    for k, mx in enumerate((top, top // 2, top // 16, top // 32, top // 16, top // 2, top // 4)):
        hs = [int(h) for h in rng.choice(pool, 1500, replace=False) if h <= mx]
        queries.append(mk(pkg, hs, {h: 1 + h % 7 for h in hs} if k % 2 else None, max_hash=mx))
    for kw in (dict(), dict(threshold_bp=2000, max_rows=4)):
        many = index.gather_many(queries, downsample=True, **kw)
        for k, q in enumerate(queries):
            one = index.gather(q, downsample=True, **kw)
            assert same(many[k], one), (kw, k)
        assert len(many[0].rows) >= 3 and len(many[3].assigned) < len(many[2].assigned) < len(many[0].assigned)


# ---------------------------------------------------------------------------------- 13: the pool

def test_pool_bytes_return(pkg):
    """The work memory comes from the device block pool and goes back there.  One call of the same shape goes first: it
    creates the blocks the pool has never seen, and builds the index's directory (which the index keeps, outside the pool)."""
    rng = np.random.default_rng(9)
    universe = [int(x) for x in rng.integers(0, M64, 3000, dtype=np.uint64)]
    sketches = [[int(x) for x in rng.choice(universe, 200, replace=False)] for _ in range(40)]
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    queries = [mk(pkg, rng.choice(universe, 1500, replace=False)) for _ in range(4)]
    L = pkg.lib()
    run_many(index, queries)
    before = L.smh_pool_bytes()
    for _ in range(3):
        got = run_many(index, queries)
        assert all(len(rows) > 5 for rows, _ in got)
        assert L.smh_pool_bytes() == before


def test_the_kernels_ran(pkg):
    L = pkg.lib()
    index = pkg.index.ResidentIndex([mk(pkg, [1, 2, 3]), mk(pkg, [3, 4])])
    L.smh_profile_enable(1)
    try:
        L.smh_profile_reset()
        run_many(index, [mk(pkg, [1, 2, 3, 4]), mk(pkg, [4])])
        assert count(pkg, "gather_many_probe") == 1 and count(pkg, "gather_many_fill") == 1 and count(pkg, "gather_many_rounds") == 1
        assert count(pkg, "gather_hits") == 0, "the batch went through the single-query route"
    finally:
        L.smh_profile_enable(0)
