"""Gather on the device (smh_index_gather, ResidentIndex.gather) against the plain-Python restatement: rows and `assigned`
must be EQUAL -- every output is an integer."""
import ctypes as C

import numpy as np
import pytest

import gather_restatement as GR

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
FIELDS = ("match", "common_remaining", "common_original", "size_match", "abund_sum")


def mk(pkg, hashes, abunds=None, max_hash=M64, track=False, ksize=21, seed=42, protein=False, num=0):
    """a sketch holding `hashes`; abunds ({hash: abundance}) makes it track abundances"""
    mh = pkg.KmerMinHash(num, ksize, protein, seed, max_hash, track or abunds is not None)
    h = sorted(int(x) for x in hashes)
    if abunds is not None:
        mh.add_many_with_abund([(x, abunds[x]) for x in h])
    elif h:
        mh.add_many(np.array(h, dtype=np.uint64))
    return mh


def as_dicts(rows):
    return [{f: getattr(r, f) for f in FIELDS} for r in rows]


def run(index, q, threshold=0, capacity=None):
    """(rows as dicts, assigned as list) with threshold_common and the capacity handed over as they are (scaled = 1)"""
    res = index.gather(q, threshold_bp=threshold, scaled=1, max_rows=capacity)
    return as_dicts(res.rows), res.assigned.tolist()


def check(pkg, sketches, query, abunds=None, threshold=0, capacity=None, expect=None):
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    got = run(index, mk(pkg, query, abunds), threshold, capacity)
    exp = expect if expect is not None else GR.gather(sketches, query, abunds, threshold, capacity)
    assert got[0] == exp[0]
    assert got[1] == exp[1]
    return got


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


# ---------------------------------------------------------------------------------- the committed fixture

class Fixture:
    def __init__(self, pkg, sketches):
        self.mins = [s["mins"] for s in sketches]
        self.max_hash = sketches[0]["max_hash"]
        self.ab = {}                                   # the query's abundances: per hash, the sum over the fixture sketches
        for s in sketches:
            for h, a in zip(s["mins"], s["abundances"]):
                self.ab[h] = self.ab.get(h, 0) + a
        self.query = sorted(self.ab)
        self.nodes = [mk(pkg, s["mins"], dict(zip(s["mins"], s["abundances"])), max_hash=self.max_hash) for s in sketches]
        self.index = pkg.index.ResidentIndex(self.nodes)
        self.q_abund = mk(pkg, self.query, self.ab, max_hash=self.max_hash)
        self.q_flat = mk(pkg, self.query, max_hash=self.max_hash)
        self._exp = {}

    def expected(self, with_abund, threshold, capacity=None):
        """one full restatement run per (abundances, threshold); a capacity cuts it (gather_restatement.cut)"""
        key = (with_abund, threshold)
        if key not in self._exp:
            self._exp[key] = GR.gather(self.mins, self.query, self.ab if with_abund else None, threshold)
        rows, assigned = self._exp[key]
        return (rows, assigned) if capacity is None else GR.cut(rows, assigned, capacity)


@pytest.fixture(scope="module")
def fx(pkg, sbt_subset_sketches):
    return Fixture(pkg, sbt_subset_sketches)


@pytest.mark.parametrize("with_abund", [True, False])
@pytest.mark.parametrize("threshold", [1, 50])
def test_fixture_rows_and_assignment(fx, with_abund, threshold):
    q = fx.q_abund if with_abund else fx.q_flat
    for cap in (0, 1, 98, 99, 1000):
        got = run(fx.index, q, threshold, cap)
        exp = fx.expected(with_abund, threshold, cap)
        assert got[0] == exp[0], cap
        assert got[1] == exp[1], cap
    full = fx.expected(with_abund, threshold)[0]
    assert len(full) == (99 if threshold == 1 else 82)
    if with_abund:
        assert any(r["abund_sum"] != r["common_remaining"] for r in full)   # the abundances are really in play


@pytest.mark.parametrize("with_abund", [True, False])
def test_fixture_derived_values(pkg, fx, with_abund):
    """the wrapper's floats are the restatement's formulas on the restatement's integers; threshold_bp goes through scaled"""
    q = fx.q_abund if with_abund else fx.q_flat
    scaled = pkg.index.scaled_of_max_hash(fx.max_hash)
    assert scaled == 2000
    res = fx.index.gather(q, threshold_bp=99_500)            # ceil(99500 / 2000) = 50
    rows, assigned = fx.expected(with_abund, 50)
    assert as_dicts(res.rows) == rows and res.assigned.tolist() == assigned
    q_ab = [fx.ab[h] for h in fx.query] if with_abund else None
    exp = GR.derived(rows, assigned, len(fx.query), q_ab, scaled)
    a = np.array(assigned)
    w = np.array(q_ab if with_abund else [1] * len(fx.query), dtype=np.uint64)
    for r, (got, e) in enumerate(zip(res.rows, exp)):
        for k, v in e.items():
            assert getattr(got, k) == v, (r, k)
        assert got.median_abund == float(np.median(w[a == r])) and got.std_abund == float(np.std(w[a == r])), r
    assert res.assigned.dtype == np.uint32


def test_query_resident_on_the_device(pkg, fx):
    """a query whose state lives in HBM is read there: same result, nothing copied to the host"""
    reps = np.repeat(np.array(fx.query, dtype=np.uint64), [fx.ab[h] for h in fx.query])
    one = pkg.KmerMinHash(0, 21, False, 42, fx.max_hash, True)       # one bulk fold: hashes + run starts
    one.add_many(reps)
    two = mk(pkg, fx.query, fx.ab, max_hash=fx.max_hash)             # a host state moved to HBM: hashes + u64 counts
    assert two.export_dev() == len(fx.query)
    flat = pkg.KmerMinHash(0, 21, False, 42, fx.max_hash, False)     # no abundances: the whole wrapper needs nothing on the host
    flat.add_many(np.array(fx.query, dtype=np.uint64))
    pkg.lib().smh_profile_reset()
    before = count(pkg, "sketch_to_host")
    for q, with_abund in ((one, True), (two, True), (flat, False)):
        res = fx.index.gather(q, threshold_bp=1, scaled=1, abund_stats=False)
        exp = fx.expected(with_abund, 1)
        assert as_dicts(res.rows) == exp[0] and res.assigned.tolist() == exp[1]
    res = fx.index.gather(flat, threshold_bp=1, scaled=1)
    assert res.rows[0].median_abund == 1.0 and res.rows[0].std_abund == 0.0
    assert count(pkg, "sketch_to_host") == before, "gather brought a device-resident query to the host"
    # they were resident: looking at one moves it now
    assert one.mins == fx.query and one.abunds == [fx.ab[h] for h in fx.query]
    assert count(pkg, "sketch_to_host") == before + 1
    assert two.abunds == [fx.ab[h] for h in fx.query]


def test_second_witness_most_common_loop(pkg, fx):
    """independent of the new kernels: arg-max by ResidentIndex.most_common, removal on the host"""
    remaining = np.array(fx.query, dtype=np.uint64)
    seq = []
    while remaining.size:
        q = pkg.KmerMinHash(0, 21, False, 42, fx.max_hash, False)
        q.add_many(remaining)
        pos, common = fx.index.most_common(q)
        if common < 1:
            break
        seq.append((pos, common))
        remaining = np.setdiff1d(remaining, np.array(fx.mins[pos], dtype=np.uint64), assume_unique=True)
    got, _ = run(fx.index, fx.q_flat, 1)
    assert [(r["match"], r["common_remaining"]) for r in got] == seq and len(seq) == 99


# ---------------------------------------------------------------------------------- shapes

def pick(rng, seq, k):
    """k distinct members of a list of Python ints (indices are drawn: numpy would turn 2^64 - 1 next to 0 into a float)"""
    return [seq[i] for i in rng.choice(len(seq), k, replace=False)]


def test_wave_and_step_edges(pkg):
    rng = np.random.default_rng(11)
    pool = sorted({0, M64} | set(int(x) for x in rng.integers(1, M64, 400, dtype=np.uint64)))
    inner = pool[1:-1]
    for lq, single in ((1, 0), (1, M64), (63, None), (64, None), (65, None)):
        query = [single] if lq == 1 else sorted([0, M64] + pick(rng, inner[:200], lq - 2))
        sketches = []
        for la in (0, 1, 63, 64, 65, 128, 129):
            if la == 0:
                s = []
            elif la == 1:
                s = [M64]
            else:   # both ends of hash space, some of the query, the rest from outside it
                s = {0, M64} | set(pick(rng, query, min(len(query), la // 3)))
                outside = [h for h in inner[200:] if h not in s]
                s = sorted(s | set(pick(rng, outside, la - len(s))))
                assert len(s) == la
            sketches.append(s)
        got = check(pkg, sketches, query)
        assert len(got[0]) >= 1


def test_query_larger_than_any_lds(pkg):
    """40 000 hashes = 320 KB: the search must finish in global memory below the sampled top"""
    rng = np.random.default_rng(5)
    allh = np.unique(rng.integers(0, M64, 90_000, dtype=np.uint64))
    query = allh[:40_000 * 2:2][:40_000]
    outside = np.setdiff1d(allh, query)
    assert query.size == 40_000
    sketches = []
    for i in range(300):
        la = int(rng.integers(50, 501))
        k = int(rng.integers(0, la + 1)) if i % 7 else la
        s = np.concatenate([rng.choice(query, k, replace=False), rng.choice(outside, la - k, replace=False)])
        sketches.append([int(x) for x in s])
    ab = {int(h): int(a) for h, a in zip(query, rng.integers(1, 1000, query.size))}
    got = check(pkg, sketches, [int(x) for x in query], ab, threshold=3)
    assert len(got[0]) > 100


def test_one_hash_held_by_every_sketch(pkg):
    """an inverted list as long as the index (3 000 sketches + 10 duplicates of the first): walked by a wave.  The first 600
    sketches also hold private hashes, 600 - i of them, which forces their order; the others hold the shared hash alone and
    have nothing left after round 0; the duplicates of sketch 0 never appear."""
    n, priv = 3000, 600
    shared = 1 << 63
    sketches, nxt = [], 1
    for i in range(n):
        k = max(0, priv - i)
        sketches.append([shared] + list(range(nxt, nxt + k)))
        nxt += k
    sketches += [list(sketches[0]) for _ in range(10)]
    query = sorted(set().union(*sketches))
    got = check(pkg, sketches, query)
    assert [r["match"] for r in got[0]] == list(range(priv))
    assert got[0][0]["common_remaining"] == priv + 1 and got[0][1]["common_remaining"] == priv - 1


def test_rounds_across_read_backs(pkg):
    B = pkg.lib().smh_gather_rounds_per_sync()
    rng = np.random.default_rng(3)
    for rounds, cap in ((B - 1, None), (B, None), (B + 1, None), (3 * B + 1, None), (3 * B + 1, B)):
        sizes = list(range(rounds, 0, -1))                 # disjoint, strictly decreasing: exactly `rounds` rounds
        order = rng.permutation(rounds)
        sketches, nxt = [None] * rounds, 10
        for rank, slot in enumerate(order):
            sketches[slot] = list(range(nxt, nxt + sizes[rank]))
            nxt += sizes[rank]
        sketches += [[nxt + 5, nxt + 6], []]               # shares nothing; empty
        query = list(range(10, nxt))
        got = check(pkg, sketches, query, capacity=cap)
        assert len(got[0]) == (rounds if cap is None else cap)
        assert [r["match"] for r in got[0]] == [int(s) for s in order[:len(got[0])]]


def test_zero_rows(pkg):
    some = [[1, 2, 3], [3, 4], []]
    assert check(pkg, [], [1, 2]) == ([], [GR.UNASSIGNED] * 2)
    assert check(pkg, some, []) == ([], [])
    assert check(pkg, some, [10, 11, 12]) == ([], [GR.UNASSIGNED] * 3)
    assert check(pkg, some, [1, 2, 3, 4], threshold=4) == ([], [GR.UNASSIGNED] * 4)
    assert check(pkg, [[], []], [1]) == ([], [GR.UNASSIGNED])


def test_errors(pkg):
    nodes = [mk(pkg, [1, 2, 3]), mk(pkg, [3, 4])]
    index = pkg.index.ResidentIndex(nodes)
    q = mk(pkg, [1, 2, 3, 4])
    assert len(run(index, q)[0]) == 2
    # only scaled sketches: a num query, a num node (that index still serves find)
    with pytest.raises(pkg.SourmashError) as ei:
        index.gather(mk(pkg, [1, 2], num=5, max_hash=M64), scaled=1)
    assert ei.value.code == 3 and "gather" in ei.value.message and "scaled" in ei.value.message
    mixed = pkg.index.ResidentIndex(nodes + [mk(pkg, [1, 2, 9], num=5, max_hash=M64)])
    with pytest.raises(pkg.SourmashError) as ei:
        mixed.gather(q, scaled=1)
    assert ei.value.code == 3 and "gather" in ei.value.message and "scaled" in ei.value.message
    assert mixed.find(q, 0.4) == [0, 1]
    # check_compatible against the nodes, with its four codes
    for code, kw in ((101, dict(ksize=31)), (102, dict(protein=True)), (103, dict(max_hash=1 << 62)), (104, dict(seed=43))):
        with pytest.raises(pkg.SourmashError) as ei:
            index.gather(mk(pkg, [1, 2], **kw), scaled=1)
        assert ei.value.code == code, kw
    # nodes that disagree among themselves: the first one that refuses the query decides
    odd = pkg.index.ResidentIndex([nodes[0], mk(pkg, [3, 4], seed=43)])
    with pytest.raises(pkg.SourmashError) as ei:
        odd.gather(q, scaled=1)
    assert ei.value.code == 104
    # rows == NULL with room asked for
    L = pkg.lib()
    n_rows = C.c_uint32(5)
    L.sourmash_err_clear()
    assert L.smh_index_gather(index._h, q._p, 1, None, 4, C.byref(n_rows), None) != 0
    with pytest.raises(pkg.SourmashError):
        pkg.errors.check()
    assert n_rows.value == 0
    assert L.smh_index_gather(index._h, q._p, 1, None, 0, C.byref(n_rows), None) == 0 and n_rows.value == 0


def test_pool_bytes_return(pkg):
    """Gather's memory comes from the device block pool and goes back there.  A block the pool has never seen is created
    by the first call that needs it and parked when that call ends, so one call of the same shape goes first; after it the
    pool must stand where it stood, call after call."""
    rng = np.random.default_rng(9)
    universe = [int(x) for x in rng.integers(0, M64, 3000, dtype=np.uint64)]
    sketches = [[int(x) for x in rng.choice(universe, 200, replace=False)] for _ in range(40)]
    index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
    queries = [mk(pkg, rng.choice(universe, 1500, replace=False)) for _ in range(4)]
    L = pkg.lib()
    run(index, queries[0])
    before = L.smh_pool_bytes()
    for q in queries:
        rows, _ = run(index, q)
        assert len(rows) > 5
        assert L.smh_pool_bytes() == before
