"""Collapsing a resident index by groups on the device (smh_index_collapse; ResidentIndex.collapse) and the read-back
(smh_index_read) against the plain-Python restatement: every output is an integer, so offsets, hashes and abundances must be
EQUAL.  Host KmerMinHash.merge is the second witness of the union.  The shapes stand on both sides of the sizes
smh_collapse_geometry reports; nothing here needs more than a few thousand nodes of a dozen hashes, apart from the committed
fixture.

Not run at its size: the hash directory's own refusal of an index of 2^31 hashes (16 GiB of hashes); the call is the
check_directory_size every route through the directory makes."""
import ctypes as C

import numpy as np
import pytest

import collapse_restatement as CO

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
MODES = {"flat": CO.FLAT, "sum": CO.SUM, "count": CO.COUNT}
BIG = 3000   # owners of the longest planted list


def mk(pkg, sketch, max_hash=M64, ksize=21, seed=42, protein=False, num=0, track=None):
    """a sketch holding `sketch`: a list of hashes, or of (hash, abundance) pairs (it then tracks abundances)"""
    sketch = sorted(sketch)
    weighted = bool(sketch) and isinstance(sketch[0], tuple)
    mh = pkg.KmerMinHash(num, ksize, protein, seed, max_hash, weighted if track is None else track)
    if weighted:
        mh.add_many_with_abund(sketch)
    elif sketch:
        mh.add_many(np.array(sketch, dtype=np.uint64))
    return mh


def index_of(pkg, sketches, **kw):
    return pkg.index.ResidentIndex([mk(pkg, s, **kw) for s in sketches])


def flat(sketches):
    return [[x[0] if isinstance(x, tuple) else x for x in s] for s in sketches]


def same(child, want, what=""):
    off, h, ab = child.read()
    assert off.dtype == np.uint64 and h.dtype == np.uint64 and (ab is None or ab.dtype == np.uint32)
    assert off.tolist() == want[0], what
    assert h.tolist() == want[1], what
    assert (ab is None) == (want[2] is None) and (ab is None or ab.tolist() == want[2]), what


def check(index, sketches, group, G, min_count=1, min_fraction=0.0, abund="flat"):
    """collapse on the device == the restatement; `sketches` is what the index holds"""
    child = index.collapse(group, G, min_count, min_fraction, abund)
    what = "G=%d min_count=%d min_fraction=%r %s" % (G, min_count, min_fraction, abund)
    same(child, CO.collapse(sketches if abund == "sum" else flat(sketches), group, G, min_count, min_fraction, MODES[abund]), what)
    assert len(child) == G and child.has_abundances == (abund != "flat") and not child.has_taxonomy
    assert child.sizes().tolist() == np.diff(child.read()[0]).tolist()
    return child


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


def u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def raw(pkg, index, group, G, min_count=1, min_fraction=0.0, abund=0):
    """the C call itself: (handle or None, error code, message)"""
    L = pkg.lib()
    L.sourmash_err_clear()
    g = None if group is None else np.ascontiguousarray(group, dtype=np.uint32)
    h = L.smh_index_collapse(index._h if index is not None else None, u32p(g) if g is not None else None, G, min_count, min_fraction, abund)
    code, msg = 0, ""
    try:
        pkg.errors.check()
    except pkg.SourmashError as e:
        code, msg = e.code, e.message
    if h is not None:
        L.smh_index_free(h)
    return h, code, msg


@pytest.fixture(scope="module")
def geometry(pkg):
    lane_max, wave_max, tile = pkg.matrix.collapse_geometry()
    assert 2 <= lane_max < 63 and 65 < wave_max < BIG - 1 and 64 < tile and 2 * tile + 1 < 2 * BIG
    return lane_max, wave_max, tile


# ---------------------------------------------------------------------------------- the committed fixture

class Fixture:
    def __init__(self, pkg, sketches):
        self.max_hash = sketches[0]["max_hash"]
        self.sketches = [list(zip(s["mins"], s["abundances"])) for s in sketches]
        self.nodes = [mk(pkg, s, max_hash=self.max_hash) for s in self.sketches]
        self.index = pkg.index.ResidentIndex(self.nodes)
        self.mod7 = [i % 7 for i in range(len(sketches))]
        self.clustering = self.index.cluster(0.01, "max_containment")


@pytest.fixture(scope="module")
def fx(pkg, sbt_subset_sketches):
    return Fixture(pkg, sbt_subset_sketches)


@pytest.mark.parametrize("abund", ["flat", "sum", "count"])
@pytest.mark.parametrize("min_fraction", [0.0, 0.5, 1.0])
def test_fixture(fx, abund, min_fraction):
    check(fx.index, fx.sketches, fx.mod7, 7, 1, min_fraction, abund)
    cl = fx.clustering
    assert 1 < cl.n_clusters < 100
    child = fx.index.collapse(cl, min_fraction=min_fraction, abund=abund)
    same(child, CO.collapse(fx.sketches if abund == "sum" else flat(fx.sketches), cl.cluster.tolist(), cl.n_clusters, 1, min_fraction,
                            MODES[abund]))


def test_union_equals_host_merge(pkg, fx):
    merged = []
    for g in range(7):
        members = [m for i, m in enumerate(flat(fx.sketches)) if i % 7 == g]
        mh = mk(pkg, members[0], max_hash=fx.max_hash)
        for other in members[1:]:
            mh.merge(mk(pkg, other, max_hash=fx.max_hash))
        merged.append(mh)
    child = fx.index.collapse(fx.mod7, 7)
    off, h, _ = child.read()
    for g in range(7):
        assert h[int(off[g]):int(off[g + 1])].tolist() == merged[g].mins
    out = child.compare(pkg.index.ResidentIndex(merged), want=("common", "size", "jaccard"))
    assert (np.diag(out["common"]) == np.diag(out["size"])).all() and (np.diag(out["jaccard"]) == 1.0).all()
    assert np.diag(out["common"]).tolist() == [len(m) for m in merged]


# ---------------------------------------------------------------------------------- owner lists and groups at the kernels' edges

class Planted:
    """BIG + 100 nodes of three private hashes each; for every length L of `lengths` one planted hash held by nodes 0 .. L - 1,
    so its owner list is exactly L long.  Abundances: 1 + (v + hash) % 5."""

    def __init__(self, pkg, lengths):
        self.n = BIG + 100
        self.lengths = lengths
        self.sketches = []
        for v in range(self.n):
            held = [(1 << 40) + 4 * v + k for k in range(3)] + [(1 << 63) + L for L in lengths if v < L]
            self.sketches.append([(h, 1 + (v + h) % 5) for h in held])
        self.index = index_of(pkg, self.sketches)


@pytest.fixture(scope="module")
def planted(pkg, geometry):
    lane_max, wave_max, _ = geometry
    return Planted(pkg, sorted({lane_max - 1, lane_max, lane_max + 1, 63, 64, 65, wave_max, wave_max + 1, BIG}))


@pytest.mark.parametrize("abund", ["flat", "sum", "count"])
def test_owner_lists_in_one_group(planted, abund):
    p = planted
    check(p.index, p.sketches, [0] * p.n, 1, abund=abund)
    # every planted hash is kept exactly when its list is long enough: the counts are exact in every regime
    for L in p.lengths:
        child = check(p.index, p.sketches, [0] * p.n, 1, min_count=L, abund=abund)
        assert child.read()[1].tolist() == [(1 << 63) + x for x in p.lengths if x >= L]
    check(p.index, p.sketches, [1] * p.n, 3, min_count=2, abund=abund)   # empty groups first and last


@pytest.mark.parametrize("abund", ["flat", "sum", "count"])
def test_owner_lists_in_two_groups(planted, abund):
    p = planted
    check(p.index, p.sketches, [v % 2 for v in range(p.n)], 2, abund=abund)
    check(p.index, p.sketches, [v % 2 for v in range(p.n)], 2, min_count=32, abund=abund)
    check(p.index, p.sketches, [1 - v % 2 for v in range(p.n)], 2, min_count=33, abund=abund)
    # two groups with a dropped node between every pair of members
    check(p.index, p.sketches, [None if v % 3 == 1 else v % 3 // 2 for v in range(p.n)], 2, min_count=2, abund=abund)


@pytest.mark.parametrize("abund", ["flat", "sum", "count"])
def test_one_owner_per_group_is_the_identity(planted, abund):
    p = planted
    child = check(p.index, p.sketches, list(range(p.n)), p.n, abund=abund)
    off, h, ab = p.index.read()
    got = child.read()
    assert got[0].tolist() == off.tolist() and got[1].tolist() == h.tolist()
    if abund == "sum":
        assert got[2].tolist() == ab.tolist()
    # reversed against node order
    check(p.index, p.sketches, list(range(p.n - 1, -1, -1)), p.n, abund=abund)
    assert check(p.index, p.sketches, list(range(p.n)), p.n, min_count=2, abund=abund).read()[1].size == 0


@pytest.mark.parametrize("abund", ["sum", "count"])
def test_group_tiles(planted, geometry, abund):
    """the BIG-owner list spread over G groups, with G on both sides of the tile of LDS counters and across two of its borders"""
    p, tile = planted, geometry[2]
    for G in (tile - 1, tile, tile + 1, 2 * tile + 1):
        group = [v % G for v in range(p.n)]
        check(p.index, p.sketches, group, G, abund=abund)
        check(p.index, p.sketches, group, G, min_count=2, abund=abund)
        # interleaved: neighbouring nodes lie a tile apart
        check(p.index, p.sketches, [(v * tile + v // 2) % G for v in range(p.n)], G, abund=abund)
    # the owners at both ends of a wide range of groups: the tiles between hold nothing, empty groups in the middle
    G = 5 * tile
    check(p.index, p.sketches, [G - 1 - v % 3 if v % 2 else v % 3 for v in range(p.n)], G, min_count=2, abund=abund)


def test_every_node_dropped_and_empty_shapes(pkg, planted):
    p = planted
    child = check(p.index, p.sketches, [None] * p.n, 4, abund="count")
    assert child.read()[0].tolist() == [0] * 5
    empty = pkg.index.ResidentIndex([])
    same(empty.collapse([], 3), ([0, 0, 0, 0], [], None))
    same(empty.collapse([], 2, abund="sum"), ([0, 0, 0], [], []))
    hollow = index_of(pkg, [[], []])
    same(hollow.collapse([0, 1], 2, abund="count"), ([0, 0, 0], [], []))


# ---------------------------------------------------------------------------------- need_g

def test_need(pkg):
    rng = np.random.default_rng(5)
    universe = [int(x) for x in rng.integers(1, M64, 30, dtype=np.uint64)]
    sketches = [sorted(rng.choice(universe, 15, replace=False).tolist()) for _ in range(10)]
    group = [0, 1, 1, 2, 2, 2, 3, 3, 3, 3]   # sizes 1, 2, 3, 4 in one call
    index = index_of(pkg, sketches)
    for fraction in (0.5, 1.0, 2 / 3, 0.28):
        check(index, sketches, group, 4, 1, fraction, "count")
    child = check(index, sketches, group, 4, min_count=3)            # above m_g for the groups of 1 and 2: empty
    assert child.sizes()[0] == 0 and child.sizes()[1] == 0 and child.sizes()[3] > 0
    check(index, sketches, group, 4, min_count=2, min_fraction=0.0, abund="count")
    check(index, sketches, group, 4, min_count=5)                    # above every m_g
    check(index, sketches, group, 4, min_count=0xFFFFFFFF)
    check(index, sketches, [3, 0, 3, 0, 3, 0, 3, 0, 3, 0], 4, 1, 0.5)   # empty groups in the middle


def test_hash_order_is_unsigned(pkg):
    lo, hi = (1 << 63) - 1, 1 << 63
    sketches = [[hi, M64, 5], [1, lo, hi + 1], [lo, M64]]
    index = index_of(pkg, sketches)   # (max_hash = 2^64 - 1)
    child = check(index, sketches, [0, 0, 0], 1)
    assert child.read()[1].tolist() == [1, 5, lo, hi, hi + 1, M64]
    check(index, sketches, [1, 0, 1], 2, min_fraction=1.0, abund="count")
    assert child.max_hash == M64


# ---------------------------------------------------------------------------------- abundances

TOP = (1 << 32) - 1


def test_sum_keeps_2_32_minus_1_and_refuses_2_32(pkg):
    sketches = [[(7, TOP - 1), (9, 1)], [(7, 1), (9, 2)]]
    index = index_of(pkg, sketches)
    child = check(index, sketches, [0, 0], 1, abund="sum")
    assert child.read()[2].tolist() == [TOP, 3]
    # groups 1 and 2 both hold a sum of 2^32: the lowest is named; group 0 is fine
    over = [[(7, 1)], [(7, TOP)], [(7, 1)], [(9, TOP)], [(9, 1)]]
    index = index_of(pkg, over)
    L = pkg.lib()
    for again in (False, True):   # (the first refusal parks the blocks the pool had never seen)
        pool = L.smh_pool_bytes()
        h, code, msg = raw(pkg, index, [0, 1, 1, 2, 2], 3, abund=CO.SUM)
        assert h is None and code == 3 and "group 1 " in msg and "2^32" in msg
        assert not again or L.smh_pool_bytes() == pool
    with pytest.raises(CO.Refused, match="group 1 "):
        CO.collapse(over, [0, 1, 1, 2, 2], 3, abund=CO.SUM)
    assert index.find(mk(pkg, [7]), 0.5) == [0, 1, 2]
    # the sum that overflows is not kept: no refusal; COUNT and FLAT never look at it
    check(index, over, [0, 1, 1, 2, 2], 3, min_count=3, abund="sum")
    check(index, over, [0, 1, 1, 2, 2], 3, abund="count")
    check(index, over, [0, 1, 1, 2, 2], 3, abund="flat")


def test_sum_wherever_the_abundances_live(pkg, fx):
    group = [(i * 3) % 5 for i in range(100)]
    fresh = pkg.index.ResidentIndex(fx.nodes)          # abundances still on the host
    check(fresh, fx.sketches, group, 5, abund="sum")
    fresh.norms2()                                     # ... after an angular call: in HBM
    check(fresh, fx.sketches, group, 5, 1, 0.5, abund="sum")
    mx = fx.max_hash // 3
    cut = [[(h, a) for h, a in s if h <= mx] for s in fx.sketches]
    check(fresh.downsample(max_hash=mx), cut, group, 5, abund="sum")                              # a child cut in HBM
    check(pkg.index.ResidentIndex(fx.nodes).downsample(max_hash=mx), cut, group, 5, abund="sum")   # a child cut with host abundances
    check(pkg.index.ResidentIndex(fx.nodes, max_hash=mx), cut, group, 5, 2, 0.0, abund="count")


def test_count_without_abundances_and_flat_with(pkg, fx):
    plain = index_of(pkg, flat(fx.sketches), max_hash=fx.max_hash)
    assert not plain.has_abundances
    child = check(plain, flat(fx.sketches), fx.mod7, 7, abund="count")
    assert child.has_abundances and child.read()[2].max() <= 15
    assert not check(fx.index, fx.sketches, fx.mod7, 7, abund="flat").has_abundances


# ---------------------------------------------------------------------------------- the child is a full index

def test_the_child_is_a_full_index(pkg, fx):
    child = fx.index.collapse(fx.mod7, 7, abund="sum")
    sk = child.sketches()
    assert len(sk) == 7 == len(child.nodes) and all(s.track_abundance and s.max_hash == fx.max_hash and s.ksize == 21 for s in sk)
    assert [s.mins for s in sk] == [s.mins for s in child.nodes]
    twin = pkg.index.ResidentIndex(sk)
    same(twin, tuple(x if x is None else x.tolist() for x in child.read()))
    queries = [fx.nodes[3], fx.nodes[50], sk[2]]
    for q in queries:
        assert child.find(q, 0.01) == twin.find(q, 0.01)
        assert child.find(q, 0.05, containment=True) == twin.find(q, 0.05, containment=True)
        a, b = child.gather(q), twin.gather(q)
        assert a.rows == b.rows and a.assigned.tolist() == b.assigned.tolist() and len(a.rows) > 0
    a, b = child.search_many(queries, 0.01), twin.search_many(queries, 0.01)
    assert a.offsets.tolist() == b.offsets.tolist() and a.node.tolist() == b.node.tolist() and a.common.tolist() == b.common.tolist()
    assert len(a) > 0
    a, b = child.pairwise(0.0), twin.pairwise(0.0)
    assert a.offsets.tolist() == b.offsets.tolist() and a.node.tolist() == b.node.tolist() and a.common.tolist() == b.common.tolist()
    mx = fx.max_hash // 2
    same(child.downsample(max_hash=mx), tuple(x.tolist() for x in twin.downsample(max_hash=mx).read()))
    a, b = child.angular_matrix(want=("dot", "angular")), twin.angular_matrix(want=("dot", "angular"))
    assert (a["dot"] == b["dot"]).all() and (a["angular"] == b["angular"]).all() and a["dot"].any()
    assert child.norms2().tolist() == twin.norms2().tolist()
    # collapsing a collapsed index
    held = CO.sketches_of(*(x.tolist() for x in child.read()))
    check(child, held, [0, 0, 1, 1, 2, 2, 2], 3, abund="sum")
    check(child, held, [0, 0, 1, 1, 2, 2, 2], 3, 1, 1.0, abund="count")
    grand = child.collapse([0] * 7, 1)
    assert grand.read()[1].tolist() == sorted({h for s in fx.sketches for h, _ in s})


# ---------------------------------------------------------------------------------- smh_index_read

def test_read(pkg, fx):
    L = pkg.lib()
    off, h, ab = fx.index.read()
    assert CO.sketches_of(off.tolist(), h.tolist(), ab.tolist()) == fx.sketches
    assert [s.mins for s in fx.index.sketches()] == flat(fx.sketches)
    assert [s.abunds for s in fx.index.sketches()] == [[a for _, a in s] for s in fx.sketches]
    mx = fx.max_hash // 3
    for parent in (fx.index, pkg.index.ResidentIndex(fx.nodes)):   # abundances in HBM or not, as other tests left fx.index
        got = parent.downsample(max_hash=mx).read()
        assert CO.sketches_of(*(x.tolist() for x in got)) == [[(x, a) for x, a in s if x <= mx] for s in fx.sketches]
    cut = fx.index.downsample(max_hash=mx)
    assert all(s.max_hash == mx for s in cut.sketches()) and [s.mins for s in cut.sketches()] == [n.downsample_max_hash(mx).mins for n in fx.nodes]
    # each output alone
    n, total = len(fx.index), len(h)
    o2, h2, a2 = np.zeros(n + 1, np.uint64), np.zeros(total, np.uint64), np.zeros(total, np.uint32)
    u64 = C.POINTER(C.c_uint64)
    assert L.smh_index_read(fx.index._h, o2.ctypes.data_as(u64), None, None) == 0 and o2.tolist() == off.tolist() and not h2.any()
    assert L.smh_index_read(fx.index._h, None, h2.ctypes.data_as(u64), None) == 0 and h2.tolist() == h.tolist() and not a2.any()
    assert L.smh_index_read(fx.index._h, None, None, u32p(a2)) == 0 and a2.tolist() == ab.tolist()
    assert L.smh_index_read(fx.index._h, None, None, None) == 0
    # no abundances to read
    plain = index_of(pkg, [[1, 2], [2, 3]])
    assert plain.read()[2] is None
    a3 = np.full(4, 77, np.uint32)
    assert L.smh_index_read(plain._h, None, None, u32p(a3)) == 3 and a3.tolist() == [77] * 4
    L.sourmash_err_clear()
    # a num index reads back too
    nums = pkg.index.ResidentIndex([mk(pkg, [5, 6, 7, 8], max_hash=0, num=3), mk(pkg, [1], max_hash=0, num=3)])
    assert nums.read()[0].tolist() == [0, 3, 4] and nums.read()[1].tolist() == [5, 6, 7, 1]
    assert [s.mins for s in nums.sketches()] == [[5, 6, 7], [1]] and nums.sketches()[0].num == 3


# ---------------------------------------------------------------------------------- refusals

def test_refusals(pkg):
    L = pkg.lib()
    sk = [[(1, 1), (2, 2)], [(2, 3), (3, 1)], [(9, 1)]]
    index = index_of(pkg, sk)
    ok = [0, 1, 1]
    index.collapse(ok, 2, abund="sum")   # (builds the directory and moves the abundances: the refusals below find both in place)
    plain = index_of(pkg, flat(sk))
    wide = index_of(pkg, [[(1, 1)], [(1, 2), (5, 1 << 32)]])
    num = pkg.index.ResidentIndex([mk(pkg, [1, 2]), mk(pkg, [1, 2, 3], max_hash=0, num=2)])
    ksizes = pkg.index.ResidentIndex([mk(pkg, [1, 2]), mk(pkg, [1, 2]), mk(pkg, [2], ksize=31)])
    scaleds = pkg.index.ResidentIndex([mk(pkg, [1, 2], max_hash=1 << 60), mk(pkg, [2], max_hash=1 << 59)])
    nan = float("nan")
    cases = [
        (plain, ok, 2, 1, 0.0, CO.SUM, "does not track abundances"),
        (wide, [0, 0], 1, 1, 0.0, CO.SUM, "node 1 holds an abundance of 2^32"),
        (num, [0, 0], 1, 1, 0.0, CO.FLAT, "node 1 is not a scaled sketch"),
        (ksizes, [0, 0, 0], 1, 1, 0.0, CO.FLAT, "node 2 differs"),
        (scaleds, [0, 0], 1, 1, 0.0, CO.COUNT, "node 1 differs"),
        (index, ok, 0, 1, 0.0, CO.FLAT, "n_groups is 0"),
        (index, [0, 1, 2], 2, 1, 0.0, CO.FLAT, "group[2] is 2"),
        (index, [0, 0xFFFFFFFE, 1], 2, 1, 0.0, CO.FLAT, "group[1] is 4294967294"),
        (index, ok, 2, 1, -0.1, CO.FLAT, "min_fraction"),
        (index, ok, 2, 1, 1.0000001, CO.FLAT, "min_fraction"),
        (index, ok, 2, 1, nan, CO.FLAT, "NaN"),
        (index, ok, 2, 1, 0.0, 3, "mode 3"),
        (index, None, 2, 1, 0.0, CO.FLAT, "group is NULL"),
        (None, ok, 2, 1, 0.0, CO.FLAT, "index is NULL"),
    ]
    for idx, group, G, min_count, fraction, abund, words in cases:
        pool = L.smh_pool_bytes()
        h, code, msg = raw(pkg, idx, group, G, min_count, fraction, abund)
        assert h is None and code == 3 and words in msg and msg.startswith("collapse: "), (msg, words)
        assert L.smh_pool_bytes() == pool, words
        if idx is index:
            assert index.find(mk(pkg, [2]), 0.0) == [0, 1], words   # the parent still answers
    # what SUM refuses the other modes take
    check(plain, flat(sk), ok, 2, abund="count")
    check(wide, [[1], [1, 5]], [0, 0], 1, abund="count")
    check(scaleds.downsample(max_hash=1 << 59), [[1, 2], [2]], [0, 0], 1, abund="flat")
    with pytest.raises(ValueError):
        index.collapse([0, 1], 2)
    with pytest.raises(ValueError):
        index.collapse([0, 1, -2], 2)


# ---------------------------------------------------------------------------------- bookkeeping

def test_bookkeeping(pkg):
    L = pkg.lib()
    rng = np.random.default_rng(11)
    universe = [int(x) for x in rng.integers(1, M64, 400, dtype=np.uint64)]
    sketches = [[(int(h), 1 + int(h) % 3) for h in rng.choice(universe, 120, replace=False)] for _ in range(40)]
    group = [v % 6 for v in range(40)]
    index = index_of(pkg, sketches)
    names = ("collapse_count", "collapse_emit", "collapse_partition", "collapse_finish")
    L.smh_profile_enable(1)
    try:
        L.smh_profile_reset()
        built, made = count(pkg, "match_directory_built"), count(pkg, "index_collapsed")
        check(index, sketches, group, 6, abund="sum")
        assert [count(pkg, k) for k in names] == [1, 1, 1, 1]
        assert check(index, sketches, group, 6, 1, 0.5, abund="count").sizes().sum() > 0
        assert [count(pkg, k) for k in names] == [2, 2, 2, 2]
        assert count(pkg, "match_directory_built") - built == 1      # once over two collapses
        assert count(pkg, "index_collapsed") - made == 2
    finally:
        L.smh_profile_enable(0)
    # the work space goes back to the pool (the children, whose arrays come from it too, are freed first)
    for abund in ("flat", "sum", "count"):
        child = index.collapse(group, 6, abund=abund)
        child = None
        before = L.smh_pool_bytes()
        for _ in range(2):
            child = index.collapse(group, 6, abund=abund)
            assert len(child) == 6
            child = None
            assert L.smh_pool_bytes() == before, abund
