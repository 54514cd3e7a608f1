"""Angular similarity on abundances on the device (smh_index_angular*, smh_angular_similarity, smh_angular_block_dev) against
the plain-Python restatement (angular_restatement.py).  What must hold: dot and norm2 EQUAL; cosine bit-equal (uint64 views);
angular within 128 * 2^-53 absolute -- with a bit-equal cosine only acos differs between the device and the restatement, and
two acos good to 16 ulp of a result <= pi move 1 - 2 acos(c) / pi by at most 2 * 16 * 2^-51 * (2 / pi) plus two roundings.
The largest difference seen is printed by every comparison (DESIGN.md 3.10 quotes it)."""
import ctypes as C

import numpy as np
import pytest

import angular_restatement as AR

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
ANG_TOL = 128 * 2.0 ** -53
seen = {"angular": 0.0}


def mk(pkg, sketch, max_hash=M64, num=0, ksize=21, seed=42, protein=False, track=True):
    """a sketch holding the hashes (and, when it tracks them, the abundances) of a dict {hash: abundance}"""
    mh = pkg.KmerMinHash(num, ksize, protein, seed, max_hash, track)
    h = sorted(sketch)
    if track:
        mh.add_many_with_abund([(x, sketch[x]) for x in h])
    elif h:
        mh.add_many(np.array(h, dtype=np.uint64))
    return mh


def same(got_dot, got_cos, got_ang, exp, what=""):
    """exp: (dot, cosine, angular) as nested lists of the same shape"""
    ed = np.array(exp[0], dtype=np.uint64).reshape(np.shape(got_dot))
    ec = np.array(exp[1], dtype=np.float64).reshape(np.shape(got_cos))
    ea = np.array(exp[2], dtype=np.float64).reshape(np.shape(got_ang))
    assert np.array_equal(np.asarray(got_dot, dtype=np.uint64), ed), what
    gc = np.ascontiguousarray(got_cos, dtype=np.float64)
    assert np.array_equal(gc.view(np.uint64), ec.view(np.uint64)), what
    diff = float(np.max(np.abs(np.asarray(got_ang, dtype=np.float64) - ea))) if ea.size else 0.0
    seen["angular"] = max(seen["angular"], diff)
    print("angular: largest |device - restatement| %.3e here, %.3e so far (bound %.3e) %s" % (diff, seen["angular"], ANG_TOL, what))
    assert diff <= ANG_TOL, what
    # the special values are exact
    ga = np.asarray(got_ang, dtype=np.float64)
    assert np.array_equal(ga[ec == 0.0], np.zeros(int((ec == 0.0).sum()))) and np.array_equal(ga[ec == 1.0], np.ones(int((ec == 1.0).sum())))


def matrix(index, other=None):
    out = index.angular_matrix(other, want=("dot", "cosine", "angular"))
    return out["dot"], out["cosine"], out["angular"]


def subset(rng, pool, k, ab_hi=1000):
    idx = rng.choice(len(pool), k, replace=False) if k else []
    return {pool[i]: int(rng.integers(1, ab_hi + 1)) for i in idx}


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


# ---------------------------------------------------------------------------------- sizes and placements

ROW_SIZES = (0, 1, 63, 64, 65, 4096, 4097, 8193)      # LDS staging: whole (shift 0), every 2nd hash, every 4th
COL_SIZES = (0, 1, 63, 64, 65, 129)


@pytest.fixture(scope="module")
def grid(pkg):
    rng = np.random.default_rng(21)
    pool = sorted({0, M64} | set(int(x) for x in rng.integers(1, M64, 12_000, dtype=np.uint64)))
    rows = [subset(rng, pool, k) for k in ROW_SIZES]
    return rng, pool, rows, pkg.index.ResidentIndex([mk(pkg, r) for r in rows])


@pytest.mark.parametrize("n_cols", [1, 3, 4, 5, 257])
def test_sizes(pkg, grid, n_cols):
    """every row size against every column size; 257 columns leave a ragged last wave and a ragged last chunk"""
    rng, pool, rows, rindex = grid
    cols = [subset(rng, pool, COL_SIZES[(j + n_cols) % len(COL_SIZES)]) for j in range(n_cols)]
    if n_cols == 257:
        assert {len(c) for c in cols} == set(COL_SIZES)
    assert pkg.lib().smh_angular_prune_min_pairs() > len(rows) * n_cols        # the unpruned route
    cindex = pkg.index.ResidentIndex([mk(pkg, c) for c in cols])
    same(*matrix(rindex, cindex), AR.block(rows, cols), "rows x %d columns" % n_cols)
    walked, skipped = pkg.matrix.angular_last_stats()
    nonempty = sum(1 for r in rows if r) * sum(1 for c in cols if c)
    assert (walked, skipped) == (nonempty, len(rows) * n_cols - nonempty)
    if n_cols == 257:      # and the other way round: short rows, columns of thousands of hashes (129 steps per column)
        same(*matrix(cindex, rindex), AR.block(cols, rows), "257 rows x the row sizes as columns")


@pytest.mark.parametrize("row_len", [100, 5000, 9000])
def test_placement(pkg, row_len):
    """columns entirely below the row, entirely above it, interleaved with it; hashes 0 and 2^64 - 1 in both"""
    rng = np.random.default_rng(row_len)
    lo, hi = 1 << 62, 3 << 62
    mid = sorted(set(int(x) for x in rng.integers(lo, hi, 2 * row_len + 400, dtype=np.uint64)))
    row_inner = subset(rng, mid, row_len)
    below = {int(x): int(rng.integers(1, 50)) for x in rng.integers(1, lo, 150, dtype=np.uint64)}
    above = {int(x): int(rng.integers(1, 50)) for x in rng.integers(hi, M64, 150, dtype=np.uint64)}
    inter = subset(rng, mid, 300)
    ends = {0: 3, M64: 5}
    rows = [row_inner, {**row_inner, **ends}]
    cols = [below, above, inter, {**inter, **ends}, {**below, 0: 2}, {**above, M64: 7}, {0: 1}, {M64: 1}, {**ends}]
    rindex, cindex = pkg.index.ResidentIndex([mk(pkg, r) for r in rows]), pkg.index.ResidentIndex([mk(pkg, c) for c in cols])
    exp = AR.block(rows, cols)
    assert exp[0][0][0] == 0 and exp[0][0][1] == 0 and exp[0][0][2] > 0 and exp[0][1][3] > exp[0][0][3] and exp[0][1][8] == 3 * 3 + 5 * 5
    same(*matrix(rindex, cindex), exp, "placement, row of %d" % row_len)
    same(*matrix(cindex, rindex), AR.block(cols, rows), "placement transposed, columns of %d" % row_len)


# ---------------------------------------------------------------------------------- integer and rounding edges

def test_identical_sketches(pkg):
    sq = {h: a for h, a in zip((5, 9, 11, 40), (2, 4, 5, 6))}        # norm2 = 81: sqrt(81)^2 is exact
    a, b = mk(pkg, sq), mk(pkg, sq)
    assert a.angular_parts(b) == (1.0, 1.0, 81, 81, 81)
    assert a.angular_similarity(a) == 1.0
    # no such luck in general: the literal rule decides, and it stays within two ulp of 1
    rng = np.random.default_rng(4)
    for k in (3, 64, 500):
        s = subset(rng, list(range(10, 5000)), k)
        ang, cos, dot, na, nb = mk(pkg, s).angular_parts(mk(pkg, s))
        exp = AR.pair(s, s)
        assert (dot, na, nb) == exp[:3] and dot == na
        assert np.float64(cos).view(np.uint64) == np.float64(exp[3]).view(np.uint64) and 1.0 - 2.0 ** -51 <= cos <= 1.0
        assert abs(ang - exp[4]) <= ANG_TOL
    # an index against itself sets its diagonal
    idx = pkg.index.ResidentIndex([mk(pkg, {1: 1, 2: 1}), mk(pkg, {}), mk(pkg, {1: 1, 2: 1})])
    d, c, g = matrix(idx)
    assert d.tolist() == [[2, 0, 2], [0, 0, 0], [2, 0, 2]]
    assert c[0, 0] == 1.0 and g[0, 0] == 1.0 and c[1, 1] == 0.0 and g[1, 1] == 0.0 and c[2, 2] == 1.0
    same(d, c, g, AR.block([{1: 1, 2: 1}, {}, {1: 1, 2: 1}], [{1: 1, 2: 1}, {}, {1: 1, 2: 1}], symmetric=True), "small symmetric")


def test_large_abundances(pkg):
    """abundances around 2^31: dot and norm2 pass 2^53, the conversions to double round"""
    B = 1 << 31
    a = {10: B + 1, 20: B - 3, 30: B + 12345}
    b = {10: B - 1, 20: B + 7, 35: 9, 30: B - 99999}
    c = {20: (1 << 32) - 1}                               # the largest abundance there is
    sk = [a, b, c, {7: 1}]
    exp = AR.block(sk, sk)
    assert exp[0][0][1] > 1 << 53 and AR.norm2(a) > 1 << 63 and AR.norm2(c) == ((1 << 32) - 1) ** 2
    assert float(exp[0][0][1]) != exp[0][0][1]            # the dot is not a double
    idx, idx2 = pkg.index.ResidentIndex([mk(pkg, s) for s in sk]), pkg.index.ResidentIndex([mk(pkg, s) for s in sk])
    same(*matrix(idx, idx2), exp, "abundances around 2^31")
    same(*matrix(idx), AR.block(sk, sk, symmetric=True), "abundances around 2^31, symmetric")
    assert idx.norms2().tolist() == [AR.norm2(s) for s in sk]
    got = mk(pkg, a).angular_parts(mk(pkg, b))
    e = AR.pair(a, b)
    assert got[2:] == e[:3] and np.float64(got[1]).view(np.uint64) == np.float64(e[3]).view(np.uint64) and abs(got[0] - e[4]) <= ANG_TOL


def test_norm2_that_does_not_fit(pkg):
    top = (1 << 32) - 1
    ok, wide, two = {5: 7, 6: top}, {5: 1 << 32}, {5: top, 9: top}
    assert AR.norm2(ok) < 1 << 64
    for bad in (wide, two):
        with pytest.raises(AR.Norm2Overflow):
            AR.norm2(bad)
    good = pkg.index.ResidentIndex([mk(pkg, ok), mk(pkg, {5: 2})])
    assert good.norms2().tolist() == [AR.norm2(ok), 4]
    # the message names the lowest offending node, whichever kind it is
    for nodes, first in (([ok, two, ok, wide], 1), ([ok, ok, wide, two], 2), ([two], 0), ([wide], 0)):
        idx = pkg.index.ResidentIndex([mk(pkg, s) for s in nodes])
        assert idx.has_abundances
        for call in (idx.angular_matrix, idx.norms2, lambda: idx.angular(mk(pkg, ok)), lambda: good.angular_matrix(idx),
                     lambda: idx.angular_matrix(good)):
            with pytest.raises(pkg.SourmashError) as ei:
                call()
            assert ei.value.code == 3 and "node %d " % first in ei.value.message and "64 bits" in ei.value.message, ei.value.message
        assert len(idx.find(mk(pkg, ok), 0.0)) >= 1           # find is unchanged
    # a query and a pair: on the host state, and on a state that lives in HBM (u64 counts, narrowed by a kernel)
    for bad in (wide, two):
        q = mk(pkg, bad, max_hash=M64)
        for resident in (False, True):
            if resident:
                assert q.export_dev() == len(bad)
            for call in (lambda: good.angular(q), lambda: q.angular_similarity(mk(pkg, ok)), lambda: mk(pkg, ok).angular_similarity(q)):
                with pytest.raises(pkg.SourmashError) as ei:
                    call()
                assert ei.value.code == 3 and "64 bits" in ei.value.message
    # the device form
    import torch
    h = torch.tensor([5, 9, 5, 9, 5, 9], dtype=torch.int64, device="cuda")
    a = torch.tensor(np.array([3, 4, top, top, top, top], dtype=np.uint32).view(np.int32), device="cuda")
    with pytest.raises(pkg.SourmashError) as ei:
        pkg.matrix.angular_block_dev(h, a, [0, 2, 4, 6], h, a, [0, 2, 4, 6])
    assert ei.value.code == 3 and "row sketch 1 " in ei.value.message
    with pytest.raises(pkg.SourmashError) as ei:
        pkg.matrix.angular_block_dev(h, a, [0, 2], h, a, [0, 2, 4, 6])
    assert ei.value.code == 3 and "column sketch 1 " in ei.value.message


# ---------------------------------------------------------------------------------- the committed fixture, 100 x 100

class Fixture:
    def __init__(self, pkg, sketches):
        self.max_hash = sketches[0]["max_hash"]
        self.S = [dict(zip(s["mins"], s["abundances"])) for s in sketches]
        self.nodes = [mk(pkg, s, max_hash=self.max_hash) for s in self.S]
        self.index = pkg.index.ResidentIndex(self.nodes)
        self.other = pkg.index.ResidentIndex(self.nodes)
        self.literal = AR.block(self.S, self.S)                    # every pair by the formula, the diagonal included
        self.norms = [AR.norm2(s) for s in self.S]
        n = len(self.S)
        self.symmetric = [[list(r) for r in m] for m in self.literal]
        for i in range(n):
            self.symmetric[0][i][i] = self.norms[i]
            self.symmetric[1][i][i] = self.symmetric[2][i][i] = 1.0


@pytest.fixture(scope="module")
def fx(pkg, sbt_subset_sketches):
    return Fixture(pkg, sbt_subset_sketches)


def test_fixture_symmetric(pkg, fx):
    assert fx.index.has_abundances and 10_000 >= pkg.lib().smh_angular_prune_min_pairs()      # the pruned route
    d, c, a = matrix(fx.index)
    same(d, c, a, fx.symmetric, "fixture, one index")
    assert pkg.matrix.angular_last_stats() == (1398, 4950 - 1398)
    for m in (d, c, a):
        assert np.array_equal(m.view(np.uint64), m.T.view(np.uint64))
    assert np.diag(d).tolist() == fx.norms and (np.diag(c) == 1.0).all() and (np.diag(a) == 1.0).all()
    assert fx.index.norms2().tolist() == fx.norms
    only = fx.index.angular_matrix()                               # the default asks for one matrix
    assert list(only) == ["angular"] and np.array_equal(only["angular"].view(np.uint64), a.view(np.uint64))
    # the literal formula on the diagonal stays within two ulp of what the symmetric form sets
    lit = np.array([fx.literal[1][i][i] for i in range(100)])
    assert (lit <= 1.0).all() and (lit >= 1.0 - 2.0 ** -51).all()


def test_fixture_two_indexes(pkg, fx):
    d, c, a = matrix(fx.index, fx.other)
    same(d, c, a, fx.literal, "fixture, two indexes")
    assert pkg.matrix.angular_last_stats() == (2 * 1398 + 100, 10_000 - 2 * 1398 - 100)
    # find, compare and gather on an index that has served angular calls are what they were
    cc = fx.index.compare(fx.other, want=("count_common",))["count_common"]
    assert int((cc > 0).sum()) == 2 * 1398 + 100
    assert ((cc > 0) == (d > 0)).all()


def test_prune_matrix_changes_nothing(pkg, fx):
    """angular_block_dev with the count_common matrix and without it: identical outputs, different walks"""
    import torch
    flat = np.concatenate([np.array(sorted(s), dtype=np.uint64) for s in fx.S])
    ab = np.concatenate([np.array([s[h] for h in sorted(s)], dtype=np.uint32) for s in fx.S])
    off = np.zeros(101, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in fx.S])
    th = torch.from_numpy(flat.view(np.int64)).cuda()
    ta = torch.from_numpy(ab.view(np.int32)).cuda()
    cc = pkg.matrix.compare_block_dev(th, off, th, off, 0, want=("count_common",))["count_common"]
    names = ("dot", "cosine", "angular", "row_norm2", "col_norm2")
    runs = {}
    for key, prune, sym in (("full", None, False), ("pruned", cc, False), ("sym", None, True), ("sym_pruned", cc, True)):
        out = pkg.matrix.angular_block_dev(th, ta, off, th, ta, off, count_common=prune, symmetric=sym, want=names)
        torch.cuda.synchronize()
        runs[key] = ({k: v.cpu().numpy() for k, v in out.items()}, pkg.matrix.angular_last_stats())
    assert runs["full"][1] == (10_000, 0) and runs["pruned"][1] == (2 * 1398 + 100, 10_000 - 2 * 1398 - 100)
    assert runs["sym"][1] == (4950, 0) and runs["sym_pruned"][1] == (1398, 4950 - 1398)
    for a, b in (("full", "pruned"), ("sym", "sym_pruned")):
        for k in names:
            assert np.array_equal(runs[a][0][k].view(np.uint64), runs[b][0][k].view(np.uint64)), (a, k)
    o = runs["pruned"][0]
    same(o["dot"].view(np.uint64), o["cosine"], o["angular"], fx.literal, "device form")
    o = runs["sym_pruned"][0]
    same(o["dot"].view(np.uint64), o["cosine"], o["angular"], fx.symmetric, "device form, symmetric")
    assert o["row_norm2"].view(np.uint64).tolist() == fx.norms and o["col_norm2"].view(np.uint64).tolist() == fx.norms


# ---------------------------------------------------------------------------------- a query against the index, pairs

def test_every_fixture_sketch_as_query(pkg, fx):
    for i in range(0, 100):
        res = fx.index.angular(fx.nodes[i])
        same(res.dot, res.cosine, res.angular, [m[i] for m in fx.literal], "query %d" % i if i % 25 == 0 else "")
        if i == 0:
            n = sum(1 for j in range(100) if fx.literal[0][0][j])
            assert pkg.matrix.angular_last_stats() == (100, 0) and n < 100      # a query is not pruned


def test_query_built_on_the_device(pkg):
    """a query with track_abundance=True that was sketched on the device and still lives there: read in HBM, once as
    hashes + run starts (one batch), once as hashes + u64 counts (a second batch united with the first)"""
    rng = np.random.default_rng(8)
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 260_000).tobytes())
    mx = (1 << 64) // 40
    new = lambda: pkg.KmerMinHash(0, 21, False, 42, mx, True)
    nodes = []
    for i in range(6):
        n = new()
        n.add_sequences([seq[i * 30_000:i * 30_000 + 90_000], seq[i * 30_000:i * 30_000 + 20_000 + 1000 * i]], True)
        nodes.append(n)
    index = pkg.index.ResidentIndex(nodes)
    S = [dict(zip(n.mins, n.abunds)) for n in nodes]
    assert any(v > 1 for s in S for v in s.values())
    batches = ([seq[40_000:150_000], seq[60_000:100_000]], [seq[100_000:200_000], seq[90_000:120_000], seq[100_000:110_000]])
    q, twin = new(), new()
    pkg.lib().smh_profile_reset()
    for step, batch in enumerate(batches):
        q.add_sequences(batch, True)
        twin.add_sequences(batch, True)
        expq = dict(zip(twin.mins, twin.abunds))           # (this brings the twin to the host; the query stays where it is)
        twin = new()
        for b in batches[:step + 1]:
            twin.add_sequences(b, True)
        assert len(expq) > 1000 and max(expq.values()) >= 2 + step
        before = count(pkg, "sketch_to_host")
        res = index.angular(q)
        ang = [q.angular_similarity(n) for n in nodes]
        assert count(pkg, "sketch_to_host") == before, "an angular call brought a device-resident query to the host"
        exp = AR.block([expq], S)
        same(res.dot, res.cosine, res.angular, [m[0] for m in exp], "device-built query, batch %d" % step)
        assert max(abs(x - y) for x, y in zip(ang, exp[2][0])) <= ANG_TOL and sum(1 for d in exp[0][0] if d) >= 3
    assert dict(zip(q.mins, q.abunds)) == expq               # it was resident: looking at it moves it now
    assert count(pkg, "sketch_to_host") == before + 1


def test_pair_methods(pkg, fx):
    share = next((i, j) for i in range(100) for j in range(i + 1, 100) if 0 < fx.literal[1][i][j] < 1)
    apart = next((i, j) for i in range(100) for j in range(i + 1, 100) if fx.literal[0][i][j] == 0)
    for i, j in (share, apart, (3, 3)):
        a, b = fx.nodes[i], fx.nodes[j]
        ang, cos, dot, na, nb = a.angular_parts(b)
        assert (dot, na, nb) == (fx.literal[0][i][j], fx.norms[i], fx.norms[j])
        assert np.float64(cos).view(np.uint64) == np.float64(fx.literal[1][i][j]).view(np.uint64)
        assert abs(ang - fx.literal[2][i][j]) <= ANG_TOL
        assert a.angular_similarity(b) == ang == a.similarity(b) == b.similarity(a)
        assert a.similarity(b, ignore_abundance=True) == a.compare(b)
        flat = mk(pkg, fx.S[j], max_hash=fx.max_hash, track=False)
        assert a.similarity(flat) == a.compare(flat) == a.compare(b)     # one side tracks nothing: the set similarity
    assert fx.literal[2][share[0]][share[1]] != fx.nodes[share[0]].compare(fx.nodes[share[1]])


def test_num_does_not_truncate(pkg):
    """bottom-4 sketches: the shared hash lies beyond the first four of the union, compare() does not see it.  The shared
    hash is not the largest of either sketch: a full bottom-num sketch ignores a repeat of its largest hash (quirk Q3), so an
    abundance above 1 cannot be given to that one by add_many_with_abund."""
    a, b = {1: 2, 2: 1, 10: 3, 20: 1}, {3: 1, 4: 5, 10: 4, 30: 1}
    A, B = mk(pkg, a, max_hash=0, num=4), mk(pkg, b, max_hash=0, num=4)
    assert dict(zip(A.mins, A.abunds)) == a and dict(zip(B.mins, B.abunds)) == b
    assert A.compare(B) == 0.0
    ang, cos, dot, na, nb = A.angular_parts(B)
    e = AR.pair(a, b)
    assert (dot, na, nb) == e[:3] == (12, 15, 43) and cos == e[3] and abs(ang - e[4]) <= ANG_TOL and ang > 0.2
    idx = pkg.index.ResidentIndex([A, B])
    same(*matrix(idx), AR.block([a, b], [a, b], symmetric=True), "num sketches")
    assert idx.angular(A).dot.tolist() == [15, 12]


def test_index_with_a_node_that_tracks_nothing(pkg):
    a, b = mk(pkg, {1: 2, 5: 1}), mk(pkg, {1: 1, 7: 3})
    flat = mk(pkg, {1: 1, 5: 1}, track=False)
    mixed, full = pkg.index.ResidentIndex([a, flat, b]), pkg.index.ResidentIndex([a, b])
    assert mixed.has_abundances is False and full.has_abundances is True
    for call in (mixed.angular_matrix, lambda: mixed.angular_matrix(full), lambda: full.angular_matrix(mixed), mixed.norms2,
                 lambda: mixed.angular(a), lambda: full.angular(flat)):
        with pytest.raises(pkg.SourmashError) as ei:
            call()
        assert ei.value.code == 3 and "angular" in ei.value.message
    for code, kw in ((101, dict(ksize=31)), (102, dict(protein=True)), (103, dict(max_hash=1 << 62)), (104, dict(seed=43))):
        other = mk(pkg, {1: 2}, **kw)
        for call in (lambda: full.angular(other), lambda: full.angular_matrix(pkg.index.ResidentIndex([other]))):
            with pytest.raises(pkg.SourmashError) as ei:
                call()
            assert ei.value.code == code, kw
    empty = pkg.index.ResidentIndex([])
    assert empty.has_abundances and empty.angular_matrix()["angular"].shape == (0, 0) and full.angular_matrix(empty)["angular"].shape == (2, 0)
    assert full.angular(mk(pkg, {})).angular.tolist() == [0.0, 0.0]


def test_pool_bytes_return(pkg, fx):
    """the transient memory of an angular call comes from the device block pool and goes back there"""
    L = pkg.lib()
    matrix(fx.index, fx.other)
    fx.index.angular(fx.nodes[1])
    before = L.smh_pool_bytes()
    for _ in range(3):
        matrix(fx.index, fx.other)
        fx.index.angular(fx.nodes[1])
        assert L.smh_pool_bytes() == before


def test_angular_prune_and_compare_share_one_dictionary(pkg, coracle):
    """The prune pass of an index against itself and smh_index_compare go through one route and one cached dictionary:
    "index_dictionary_built" counts the builds.  72 scaled sketches in 6 families of 12: members share most of their ~50
    hashes, families share none (pairs for the prune to skip); 72 x 72 pairs take the prune and, with 72 rows, the block route."""
    rng = np.random.default_rng(72)
    pools = [sorted({int(x) + (f << 44) for x in rng.integers(1, 1 << 40, 80, dtype=np.uint64)})[:60] for f in range(6)]
    assert all(len(p) == 60 for p in pools)
    S = [subset(rng, pools[i // 12], 50) for i in range(72)]
    assert 72 * 72 >= pkg.lib().smh_angular_prune_min_pairs()
    idx = pkg.index.ResidentIndex([mk(pkg, s) for s in S])
    exp = AR.block(S, S, symmetric=True)
    hashes = [np.array(sorted(s), dtype=np.uint64) for s in S]
    o_common, o_size, o_jac = coracle.compare_matrix(hashes, hashes, 0, 21, M64)
    assert int((o_common == 0).sum()) == 72 * 72 - 6 * 12 * 12

    def angular(delta, what):
        before = count(pkg, "index_dictionary_built")
        same(*matrix(idx), exp, what)
        assert pkg.matrix.angular_last_stats()[1] > 0, what
        assert count(pkg, "index_dictionary_built") - before == delta, what

    def compare(delta, what):
        before = count(pkg, "index_dictionary_built")
        out = idx.compare(idx, want=("jaccard", "common", "size", "count_common"))
        assert np.array_equal(out["common"], o_common) and np.array_equal(out["size"], o_size), what
        assert np.array_equal(out["jaccard"].view(np.uint64), o_jac.view(np.uint64)), what
        assert np.array_equal(out["count_common"], o_common), what            # num = 0: nothing cuts the union
        assert count(pkg, "index_dictionary_built") - before == delta, what

    angular(1, "the prune builds the dictionary")
    compare(0, "compare finds it")
    with pkg.matrix.tuning(split_frequent=False):          # (restores the default tuning in a finally)
        angular(1, "built under another split_frequent: stale")
        compare(0, "compare finds the rebuilt one")
        idx.drop_dictionary()
        compare(1, "dropped: compare builds it")
