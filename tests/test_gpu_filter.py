"""Filtering a resident index on the device (smh_index_filter; ResidentIndex.filter / subtract / intersect / inflate / flatten)
and taking a subset of its nodes (smh_index_select; ResidentIndex.select) against the plain-Python restatement: every output
is an integer, so offsets, hashes and abundances of read() must be EQUAL.  The shapes stand on both sides of the sizes
smh_filter_geometry reports (T = tile, S = operand_samples); nothing here needs more than a few thousand hashes, apart from
the committed fixture.

Not run at their size: the directory's refusal of an index of 2^31 hashes, the refusal of an operand of 2^31 hashes (16 GiB
each), and a total beyond 2^32 (the 64-bit carry of the scan is reached at every size: it is the only accumulator)."""
import ctypes as C

import numpy as np
import pytest

import filter_restatement as F

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
BIG = 3000   # owners of the longest planted list
MODES = {None: F.NONE, "keep": F.KEEP_IN, "drop": F.DROP_IN}
ABUNDS = {"own": F.OWN, "flat": F.FLAT, "operand": F.OPERAND}


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
    track = any(isinstance(x, tuple) for s in sketches for x in s)   # (an empty node of a weighted index tracks too)
    return pkg.index.ResidentIndex([mk(pkg, s, track=track, **kw) for s in sketches])


def flat(sketches):
    return [[x[0] if isinstance(x, tuple) else x for x in s] for s in sketches]


def same(child, want, what=""):
    off, h, ab = child.read()
    assert off.dtype == np.uint64 and h.dtype == np.uint64 and (ab is None or ab.dtype == np.uint32)
    assert off.tolist() == want[0], what
    assert h.tolist() == want[1], what
    assert (ab is None) == (want[2] is None) and (ab is None or ab.tolist() == want[2]), what


def rule_of(mode=None, abund="own", min_abund=0, max_abund=None, min_owners=0, max_owners=None):
    return F.Rule(MODES[mode], ABUNDS[abund], min_abund, F.NO_MAX if max_abund is None else max_abund, min_owners,
                  F.NO_MAX if max_owners is None else max_owners)


def check(pkg, index, sketches, operand=None, mode=None, op_mh=None, **kw):
    """filter on the device == the restatement; `sketches` is what the index holds, `operand` the operand's list"""
    if operand is not None and op_mh is None:
        op_mh = mk(pkg, operand, track=True if kw.get("abund") == "operand" else None)
    child = index.filter(op_mh, mode, **kw)
    want = F.filter(sketches, operand, rule_of(mode, **kw), has_abunds=index.has_abundances, operand_tracks=True)
    same(child, want, "%s %r" % (mode, kw))
    assert len(child) == len(index) and child.has_abundances == (want[2] is not None)
    assert child.sizes().tolist() == np.diff(want[0]).tolist()
    return child


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


def raw(pkg, index, op_mh, rule):
    """the C call itself: (handle or None, error code, message)"""
    L = pkg.lib()
    L.sourmash_err_clear()
    r = pkg._lib.SmhFilter(*rule) if rule is not None else None
    h = L.smh_index_filter(index._h if index is not None else None, op_mh._p if op_mh is not None else None, C.byref(r) if r is not None else None)
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
    tile, samples, threads = pkg.matrix.filter_geometry()
    assert 64 < tile <= 4096 and tile % 64 == 0 and 64 < samples <= 4096 and threads % 64 == 0
    return tile, samples, threads


def universe(seed, size):
    rng = np.random.default_rng(seed)
    return sorted({int(x) for x in rng.integers(1, M64, size, dtype=np.uint64)})


def layout(seed, lengths, weighted=True):
    """nodes of the given lengths drawn from one universe one and a half times the longest: the nodes share hashes"""
    rng = np.random.default_rng(seed)
    uni = universe(seed + 1, max(16, max(lengths, default=0) * 3 // 2))
    out = []
    for v, ln in enumerate(lengths):
        hs = sorted(int(h) for h in rng.choice(uni, ln, replace=False)) if ln else []
        out.append([(h, 1 + (h + v) % 5) for h in hs] if weighted else hs)
    return out, uni


# ---------------------------------------------------------------------------------- the committed fixture

class Fixture:
    def __init__(self, pkg, sketches):
        self.max_hash = sketches[0]["max_hash"]
        self.sketches = [list(zip(s["mins"], s["abundances"])) for s in sketches]
        self.index = pkg.index.ResidentIndex([mk(pkg, s, max_hash=self.max_hash) for s in self.sketches])
        union = {}
        for s in self.sketches[::7]:
            for h, a in s:
                union[h] = union.get(h, 0) + a
        self.operand = sorted(union.items())
        self.op_mh = mk(pkg, self.operand, max_hash=self.max_hash)


@pytest.fixture(scope="module")
def fx(pkg, sbt_subset_sketches):
    return Fixture(pkg, sbt_subset_sketches)


@pytest.mark.parametrize("kw", [dict(mode="drop"), dict(mode="keep", abund="operand"), dict(max_owners=1, min_owners=1),
                                dict(mode="keep", min_abund=2, max_abund=9, min_owners=2, abund="flat")])
def test_fixture_four_ways(pkg, fx, kw):
    kw = dict(kw)
    mode = kw.pop("mode", None)
    child = check(pkg, fx.index, fx.sketches, fx.operand if mode else None, mode, op_mh=fx.op_mh if mode else None, **kw)
    assert 0 < child.sizes().sum() < fx.index.sizes().sum()


def test_thin_wrappers(pkg, fx):
    same(fx.index.subtract(fx.op_mh), F.filter(fx.sketches, fx.operand, rule_of("drop")))
    same(fx.index.intersect(fx.op_mh), F.filter(fx.sketches, fx.operand, rule_of("keep")))
    same(fx.index.inflate(fx.op_mh), F.filter(fx.sketches, fx.operand, rule_of("keep", "operand")))
    same(fx.index.flatten(), F.filter(fx.sketches, None, rule_of(abund="flat")))
    with pytest.raises(ValueError):
        fx.index.filter(fx.op_mh)
    with pytest.raises(ValueError):
        fx.index.filter(None, "keep")
    # downsample=True: operand and index meet at the coarser max_hash
    coarse = fx.max_hash // 2
    op_coarse = fx.op_mh.downsample_max_hash(coarse)
    cut = [[(h, a) for h, a in s if h <= coarse] for s in fx.sketches]
    child = fx.index.filter(op_coarse, "keep", downsample=True)
    same(child, F.filter(cut, [(h, a) for h, a in fx.operand if h <= coarse], rule_of("keep")))
    assert child.max_hash == coarse and [m.max_hash for m in child.sketches()[:3]] == [coarse] * 3


# ---------------------------------------------------------------------------------- totals, tiles, node boundaries

def test_totals_and_boundaries(pkg, geometry):
    T = geometry[0]
    shapes = [[T - 1], [T], [T + 1], [2 * T + 1], [1],
              [0, 2 * T + 5, 0, 7, 0],                 # a node over three tiles; empty nodes first, in the middle and last
              [63, 1, 1, 62, 1, 1, 0, 3],              # boundaries at mask-word positions 63 / 64 / 65 and 127 / 128 / 129
              [5] * 100 + [T - 500 + 1, 9],            # many nodes inside one tile, one boundary on the tile's edge + 1
              [T - 64, 64, 64, T - 64]]                # boundaries on a word's edge and on a tile's
    for k, lengths in enumerate(shapes):
        sketches, uni = layout(100 + k, lengths)
        index = index_of(pkg, sketches)
        assert index.sizes().tolist() == lengths
        operand = uni[::2]
        kept = check(pkg, index, sketches, operand, "keep")
        dropped = check(pkg, index, sketches, operand, "drop")
        assert (kept.sizes() + dropped.sizes()).tolist() == lengths      # complementary
        check(pkg, index, sketches, [(h, 7 + h % 3) for h in operand], "keep", abund="operand")
        check(pkg, index, sketches, min_abund=2, max_abund=4)
        check(pkg, index, sketches, min_owners=2, abund="flat")
        check(pkg, index, sketches, max_owners=1)
        check(pkg, index, sketches, operand, "drop", min_abund=5, max_owners=1)   # the conjunction; few survivors
        check(pkg, index, sketches, uni, "drop")                                    # nothing survives
        same(index.filter(), F.select(sketches, range(len(sketches))))              # everything does: the parent itself


def test_no_nodes_and_no_hashes(pkg):
    empty = pkg.index.ResidentIndex([])
    op = mk(pkg, [(1, 2), (5, 3)])
    for kw in (dict(), dict(max_owners=1), dict(abund="flat")):
        child = empty.filter(**kw)
        assert len(child) == 0 and child.read()[0].tolist() == [0]
    assert len(empty.filter(op, "keep", abund="operand")) == 0
    hollow = index_of(pkg, [[], [], []])
    check(pkg, hollow, [[], [], []], [(1, 2)], "keep", abund="operand", max_owners=1)
    check(pkg, hollow, [[], [], []], [1], "drop")
    assert hollow.filter(min_owners=2).find(mk(pkg, [1]), 0.0) == []


# ---------------------------------------------------------------------------------- the operand

def test_operand_sizes(pkg, geometry):
    S = geometry[1]
    uni = universe(7, 5 * S)
    rng = np.random.default_rng(8)
    sketches = [[(int(h), 1 + int(h) % 4) for h in sorted(rng.choice(uni, 700, replace=False).tolist())] for _ in range(3)]
    index = index_of(pkg, sketches)
    for size in (0, 1, S - 1, S, S + 1, 2 * S, 2 * S + 1, 4 * S + 3):     # shift 0, 1 and 2 of the sampled search
        operand = sorted(int(h) for h in rng.choice(uni, size, replace=False)) if size else []
        kept = check(pkg, index, sketches, operand, "keep")
        dropped = check(pkg, index, sketches, operand, "drop")
        assert (kept.sizes() + dropped.sizes()).tolist() == [700] * 3, size
        check(pkg, index, sketches, [(h, 1 + h % 1000) for h in operand], "keep", abund="operand", op_mh=None)


def test_operand_placement_and_extreme_hashes(pkg):
    lo, mid, hi = list(range(10, 200, 3)), list(range(1000, 1300, 2)), list(range(5000, 5100))
    extreme = [0, (1 << 63) - 1, 1 << 63, M64]
    sketches = [mid, sorted(mid[::2] + extreme), extreme, [0], [M64]]
    index = index_of(pkg, sketches)
    for operand in (lo, hi, mid, extreme, [0], [M64], [(1 << 63) - 1], [1 << 63], sorted(lo + extreme + hi), [1, (1 << 63) + 1, M64 - 1]):
        kept = check(pkg, index, sketches, operand, "keep")
        dropped = check(pkg, index, sketches, operand, "drop")
        assert (kept.sizes() + dropped.sizes()).tolist() == [len(s) for s in sketches]
        check(pkg, index, sketches, [(h, 3 + h % 2) for h in operand], "keep", abund="operand")
    assert index.intersect(mk(pkg, mid)).sizes().tolist() == [len(mid), len(mid[::2]), 0, 0, 0]     # operand equal to a node
    assert index.subtract(mk(pkg, lo)).sizes().tolist() == [len(s) for s in sketches]                # wholly below
    assert index.intersect(mk(pkg, hi)).sizes().sum() == 0                                           # wholly above


# ---------------------------------------------------------------------------------- the windows

def test_abundance_window_edges(pkg):
    sketches = [[(h, 1 + h % 7) for h in range(1, 300)], [(h, 1) for h in range(100, 200)], [(5, 0xFFFFFFFF), (6, 3), (7, 1)]]
    index = index_of(pkg, sketches)
    for lo, hi in ((1, 1), (2, 5), (7, 7), (7, None), (0xFFFFFFFF, None), (0, 0xFFFFFFFE), (1, None), (0, 1)):
        child = check(pkg, index, sketches, min_abund=lo, max_abund=hi)
        ab = child.read()[2]
        assert ab.size and ab.min() >= lo and ab.max() <= (F.NO_MAX if hi is None else hi)   # the edges themselves are kept
        check(pkg, index, sketches, min_abund=lo, max_abund=hi, abund="flat")
    assert check(pkg, index, sketches, min_abund=8, max_abund=0xFFFFFFFE).sizes().sum() == 0     # a window that keeps nothing


def test_owner_windows(pkg):
    # hash 1 private to node 0, 2 shared two ways, 3 three ways, 4 by all BIG nodes; every node has one private hash more
    sketches = [[4, 10 + v] for v in range(BIG)]
    sketches[0] = sorted(sketches[0] + [1, 2, 3])
    sketches[1] = sorted(sketches[1] + [2, 3])
    sketches[BIG - 1] = sorted(sketches[BIG - 1] + [3])
    index = index_of(pkg, sketches)
    for lo, hi in ((1, 1), (0, 1), (2, None), (3, 3), (2, 2), (4, BIG - 1), (BIG, BIG), (BIG, None), (BIG + 1, None), (2, BIG - 1)):
        check(pkg, index, sketches, min_owners=lo, max_owners=hi)
    assert index.filter(min_owners=3, max_owners=3).sizes().tolist() == [1, 1] + [0] * (BIG - 3) + [1]
    assert index.filter(min_owners=BIG).sizes().tolist() == [1] * BIG
    check(pkg, index, sketches, [4], "drop", min_owners=2)


# ---------------------------------------------------------------------------------- counters

def test_directory_is_built_only_for_an_owner_window(pkg):
    sketches, uni = layout(31, [40, 50, 60])
    index = index_of(pkg, sketches)
    L = pkg.lib()
    L.smh_profile_reset()
    built, made = count(pkg, "match_directory_built"), count(pkg, "index_filtered")
    check(pkg, index, sketches, uni[::3], "keep")
    check(pkg, index, sketches, uni[::3], "drop", min_abund=2, abund="flat")
    check(pkg, index, sketches, min_owners=1)            # 0 or 1 with no maximum: no window
    check(pkg, index, sketches, min_owners=0)
    assert count(pkg, "match_directory_built") == built
    check(pkg, index, sketches, max_owners=1)
    assert count(pkg, "match_directory_built") == built + 1
    check(pkg, index, sketches, min_owners=2)
    assert count(pkg, "match_directory_built") == built + 1      # kept
    assert count(pkg, "index_filtered") - made == 6
    L.smh_profile_enable(1)
    try:
        L.smh_profile_reset()
        index.filter(max_owners=1)
        assert [count(pkg, k) for k in ("filter_flag", "filter_emit")] == [1, 1]
    finally:
        L.smh_profile_enable(0)


def test_operand_resident_on_the_device(pkg):
    """an operand whose state lives in HBM is read there: same result, nothing copied to the host"""
    mx = M64 // 20
    seq = np.random.default_rng(5).choice(np.frombuffer(b"ACGT", dtype=np.uint8), 60000).tobytes()
    made, twin = pkg.KmerMinHash(0, 21, False, 42, mx, True), pkg.KmerMinHash(0, 21, False, 42, mx, True)
    for m in (made, twin):
        m.add_sequences([seq, seq[:20000]], True)        # (the second record repeats hashes: abundances 1 and 2)
    operand = list(zip(twin.mins, twin.abunds))          # (looking at the twin brings the twin to the host)
    assert len(operand) > 1000 and {a for _, a in operand} == {1, 2}
    hs = [h for h, _ in operand]
    sketches = [[(h, 1) for h in hs[::2]], [(h, 2) for h in sorted(hs[::3] + [1, 2, 3])], [(7, 1)]]
    index = index_of(pkg, sketches, max_hash=mx)
    exported = mk(pkg, operand, max_hash=mx)
    assert exported.export_dev() == len(operand)         # a host state moved to HBM: hashes + u64 counts
    pkg.lib().smh_profile_reset()
    before = count(pkg, "sketch_to_host")
    for op_mh in (made, exported):
        check(pkg, index, sketches, operand, "keep", op_mh=op_mh)
        check(pkg, index, sketches, operand, "drop", op_mh=op_mh, abund="flat")
        check(pkg, index, sketches, operand, "keep", op_mh=op_mh, abund="operand", max_owners=1)
    assert count(pkg, "sketch_to_host") == before, "filter brought a device-resident operand to the host"
    assert made.mins == hs and count(pkg, "sketch_to_host") == before + 1


# ---------------------------------------------------------------------------------- where the abundances live

def test_abundances_on_the_host_in_hbm_and_on_a_cut(pkg):
    mx = 1 << 62
    sketches, uni = layout(41, [300, 0, 450, 17])
    sketches = [[(h >> 1, a) for h, a in s] for s in sketches]      # (below 2^63: half of them survive the cut at 2^62)
    uni = [h >> 1 for h in uni]
    operand = [(h, 100 + h % 50) for h in uni[::2]]
    op_mh = mk(pkg, operand, max_hash=1 << 63)
    index = index_of(pkg, sketches, max_hash=1 << 63)

    def everything(idx, held):
        check(pkg, idx, held, operand, "keep", op_mh=op_mh)
        check(pkg, idx, held, operand, "drop", op_mh=op_mh, min_abund=2, max_abund=4)
        child = check(pkg, idx, held, operand, "keep", op_mh=op_mh, abund="operand")
        check(pkg, idx, held, abund="flat", min_abund=3)
        return child

    inflated = everything(index, sketches)                           # abundances on the host
    # the second witness of inflate: host KmerMinHash arithmetic
    off, h, ab = inflated.read()
    table = dict(zip(op_mh.mins, op_mh.abunds))
    for v, node in enumerate(index.nodes):
        common = sorted(node.intersection_hashes(op_mh)[0])
        assert h[int(off[v]):int(off[v + 1])].tolist() == common
        assert ab[int(off[v]):int(off[v + 1])].tolist() == [table[x] for x in common]
    index.angular_matrix()                                           # moves them to HBM
    everything(index, sketches)
    cut = index.downsample(max_hash=mx)                              # a child whose abundances were cut in HBM
    held = [[(x, a) for x, a in s if x <= mx] for s in sketches]
    assert 0 < sum(len(s) for s in held) < sum(len(s) for s in sketches)
    cut_op = [(x, a) for x, a in operand if x <= mx]
    check(pkg, cut, held, cut_op, "keep", op_mh=op_mh.downsample_max_hash(mx))
    check(pkg, cut, held, cut_op, "keep", op_mh=op_mh.downsample_max_hash(mx), abund="operand", min_abund=2)
    # a filtered child's abundances are resident: filter it again, and ask it for angles
    twice = index.filter(op_mh, "keep").filter(min_abund=2)
    same(twice, F.filter(F_apply(sketches, operand), None, rule_of(min_abund=2)))
    rebuilt = pkg.index.ResidentIndex(twice.sketches())
    assert np.array_equal(twice.angular_matrix()["angular"], rebuilt.angular_matrix()["angular"])
    # FLAT drops them; inflate gives a flat index the operand's
    assert not index.flatten().has_abundances and index.flatten().read()[2] is None
    plain = index_of(pkg, flat(sketches), max_hash=1 << 63)
    assert not plain.has_abundances
    check(pkg, plain, flat(sketches), operand, "keep", op_mh=op_mh, abund="operand")
    assert plain.inflate(op_mh).has_abundances


def F_apply(sketches, operand):
    keep = {h for h, _ in operand}
    return [[(h, a) for h, a in s if h in keep] for s in sketches]


# ---------------------------------------------------------------------------------- the grid cap

def test_grid_caps(pkg, geometry):
    T = geometry[0]
    sketches, uni = layout(51, [T + 3, 0, 2 * T + 1, 70, T])
    index = index_of(pkg, sketches)
    operand = [(h, 1 + h % 9) for h in uni[::2]]
    op_mh = mk(pkg, operand)
    try:
        for cap in (1, 2):
            pkg.matrix.set_grid_cap(cap)
            before = count(pkg, "grid_capped")
            check(pkg, index, sketches, operand, "keep", op_mh=op_mh, abund="operand")
            check(pkg, index, sketches, operand, "drop", op_mh=op_mh, min_abund=2, max_owners=1)
            check(pkg, index, sketches, min_owners=2, abund="flat")
            assert count(pkg, "grid_capped") > before, cap
    finally:
        pkg.matrix.set_grid_cap(0)
    assert pkg.matrix.grid_cap() == 0


# ---------------------------------------------------------------------------------- the child is an index

def gather_rows(res):
    return [(r.match, r.common_remaining, r.common_original, r.size_match, r.abund_sum) for r in res.rows], res.assigned.tolist()


def search_rows(res):
    return res.offsets.tolist(), res.node.tolist(), res.common.tolist(), res.node_size.tolist(), res.query_size.tolist()


def same_answers(pkg, child, rebuilt, queries, parent=None, node_taxon=None):
    for q in queries:
        assert child.find(q, 0.05) == rebuilt.find(q, 0.05)
        assert child.find(q, 0.1, containment=True) == rebuilt.find(q, 0.1, containment=True)
        assert gather_rows(child.gather(q, abund_stats=False)) == gather_rows(rebuilt.gather(q, abund_stats=False))
    assert search_rows(child.search_many(queries, 0.01)) == search_rows(rebuilt.search_many(queries, 0.01))
    groups = [v % 3 for v in range(len(child))]
    assert [a.tolist() for a in child.collapse(groups, 3, abund="count").read()] == [a.tolist() for a in rebuilt.collapse(groups, 3, abund="count").read()]
    lo = child.max_hash_range[0]
    assert [a.tolist() for a in child.downsample(max_hash=lo // 2).read()[:2]] == [a.tolist() for a in rebuilt.downsample(max_hash=lo // 2).read()[:2]]
    if child.has_abundances:
        assert np.array_equal(child.angular_matrix(want=("dot", "angular"))["dot"], rebuilt.angular_matrix(want=("dot", "angular"))["dot"])
        assert np.array_equal(child.angular_matrix()["angular"], rebuilt.angular_matrix()["angular"])
    if parent is not None:
        assert child.has_taxonomy
        rebuilt.set_taxonomy(parent, node_taxon)
        for a, b in zip(child.lca_counts(queries), rebuilt.lca_counts(queries)):
            assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()


def test_child_as_an_index(pkg, fx):
    parent = [0, 0, 0, 1, 1, 2]
    node_taxon = [3 + v % 3 if v % 11 else pkg.index.NO_TAXON for v in range(len(fx.index))]
    index = pkg.index.ResidentIndex([mk(pkg, s, max_hash=fx.max_hash) for s in fx.sketches])
    index.set_taxonomy(parent, node_taxon)
    queries = [mk(pkg, fx.sketches[v], max_hash=fx.max_hash) for v in (0, 13, 50)] + [fx.op_mh]
    for child in (index.subtract(queries[1]), index.inflate(fx.op_mh), index.filter(min_owners=2), index.filter(max_owners=1, abund="flat")):
        assert child.sizes().sum() > 0
        same_answers(pkg, child, pkg.index.ResidentIndex(child.sketches()), queries, parent, node_taxon)


# ---------------------------------------------------------------------------------- select

def test_select(pkg, fx):
    sketches, _ = layout(61, [30, 0, 4100, 7, 64, 1])
    index = index_of(pkg, sketches)
    n = len(sketches)
    picks = [list(range(n)), list(range(n))[::-1], [2, 2, 0, 5, 2, 1, 1], [], [1], [3]]
    for moved in (False, True):
        if moved:
            index.angular_matrix()       # the abundances live in HBM from here on
        for ids in picks:
            child = index.select(ids)
            same(child, F.select(sketches, ids), ids)
            assert len(child) == len(ids) and child.has_abundances
        mask = np.array([True, False, True, True, False, True])
        same(index.select(mask), F.select(sketches, [0, 2, 3, 5]))
        same(index.select(np.array(picks[2], dtype=np.int64)), F.select(sketches, picks[2]))
    assert np.array_equal(index.select(picks[2]).angular_matrix()["angular"],
                          pkg.index.ResidentIndex(index.select(picks[2]).sketches()).angular_matrix()["angular"])
    with pytest.raises(ValueError):
        index.select(np.array([True, False]))
    with pytest.raises(ValueError):
        index.select([-1])
    # a num-sketch index, mixed with a scaled node: it only copies, the parameters go with the nodes
    mixed = pkg.index.ResidentIndex([mk(pkg, [1, 2, 3], max_hash=0, num=3), mk(pkg, [2, 9]), mk(pkg, [5, 6, 7, 8], max_hash=0, num=500, ksize=31)])
    child = mixed.select([2, 0, 2])
    same(child, F.select([[5, 6, 7, 8], [2, 9], [1, 2, 3]], [0, 2, 0]))
    assert [(m.num, m.ksize, m.max_hash) for m in child.sketches()] == [(500, 31, 0), (3, 21, 0), (500, 31, 0)]
    assert [m.mins for m in child.sketches()] == [[5, 6, 7, 8], [1, 2, 3], [5, 6, 7, 8]]
    assert mixed.select([1]).find(mk(pkg, [2, 9, 11]), 0.5) == [0]
    nums = pkg.index.ResidentIndex([mk(pkg, [1, 2, 3], max_hash=0, num=3), mk(pkg, [2, 3, 4], max_hash=0, num=3)])
    assert nums.select([1, 0, 1]).compare(nums, want=("count_common",))["count_common"].tolist() == [[2, 3], [3, 2], [2, 3]]


def test_select_carries_the_taxonomy_and_takes_representatives(pkg, fx):
    parent = [0, 0, 0, 1, 1, 2]
    node_taxon = [3 + v % 3 if v % 11 else pkg.index.NO_TAXON for v in range(len(fx.index))]
    index = pkg.index.ResidentIndex([mk(pkg, s, max_hash=fx.max_hash) for s in fx.sketches])
    index.set_taxonomy(parent, node_taxon)
    queries = [mk(pkg, fx.sketches[v], max_hash=fx.max_hash) for v in (0, 13, 50)] + [fx.op_mh]
    ids = [99, 5, 5, 40, 0, 11, 22, 33]
    child = index.select(ids)
    same(child, F.select(fx.sketches, ids))
    same_answers(pkg, child, pkg.index.ResidentIndex(child.sketches()), queries, parent, [node_taxon[v] for v in ids])
    cl = index.cluster(0.01, "max_containment", linkage="greedy")
    reps = np.unique(cl.representative)
    assert 1 < len(reps) < len(index)
    rebuilt = pkg.index.ResidentIndex([mk(pkg, fx.sketches[int(v)], max_hash=fx.max_hash) for v in reps])
    same(index.select(reps), tuple(a.tolist() for a in rebuilt.read()))
    made = count(pkg, "index_selected")
    index.select([0])
    assert count(pkg, "index_selected") == made + 1


# ---------------------------------------------------------------------------------- refusals

def test_every_refusal(pkg):
    L = pkg.lib()
    sk = [[(1, 1), (2, 2)], [(2, 3), (3, 1)], [(9, 1)]]
    index = index_of(pkg, sk)
    index.filter(max_owners=1)   # (builds the directory: the refusals below find it in place)
    plain = index_of(pkg, flat(sk))
    wide = index_of(pkg, [[(1, 1)], [(1, 2), (5, 1 << 32)]])
    num = pkg.index.ResidentIndex([mk(pkg, [1, 2]), mk(pkg, [1, 2, 3], max_hash=0, num=2)])
    op, op_flat, op_wide = mk(pkg, [(2, 5), (9, 6)]), mk(pkg, [2, 9]), mk(pkg, [(2, 1 << 32), (9, 1)])
    op_num, op_k31, op_prot = mk(pkg, [2], max_hash=0, num=5), mk(pkg, [2], ksize=31), mk(pkg, [2], protein=True)
    op_seed, op_fine = mk(pkg, [2], seed=43), mk(pkg, [2], max_hash=1 << 60)
    R = F.Rule
    cases = [
        (index, op, None, 3, "rule is NULL"),
        (index, op, R(3), 3, "unknown operand mode 3"),
        (index, op, R(F.KEEP_IN, 3), 3, "unknown abundance mode 3"),
        (index, op, R(min_abund=3, max_abund=2), 3, "min_abund 3 exceeds max_abund 2"),
        (index, op, R(min_owners=2, max_owners=1), 3, "min_owners 2 exceeds max_owners 1"),
        (index, op, R(F.DROP_IN, F.OPERAND), 3, "SMH_FILTER_KEEP_IN"),
        (index, None, R(F.NONE, F.OPERAND), 3, "SMH_FILTER_KEEP_IN"),
        (None, op, R(), 3, "index is NULL"),
        (num, None, R(), 3, "node 1 is not a scaled sketch"),
        (index, None, R(F.KEEP_IN), 3, "operand is NULL"),
        (index, None, R(F.DROP_IN), 3, "operand is NULL"),
        (index, op_num, R(F.KEEP_IN), 3, "the operand is not a scaled sketch"),
        (index, op_k31, R(F.KEEP_IN), 101, ""),
        (index, op_prot, R(F.DROP_IN), 102, ""),
        (index, op_fine, R(F.DROP_IN), 103, ""),
        (index, op_seed, R(F.KEEP_IN), 104, ""),
        (index, op_flat, R(F.KEEP_IN, F.OPERAND), 3, "the operand does not track abundances"),
        (plain, None, R(min_abund=1), 3, "an abundance window on an index"),
        (plain, None, R(max_abund=7), 3, "an abundance window on an index"),
        (wide, None, R(), 3, "node 1 holds an abundance of 2^32 or more"),
        (wide, op, R(F.KEEP_IN, F.OPERAND, min_abund=1), 3, "node 1 holds an abundance of 2^32 or more"),
        (index, op_wide, R(F.KEEP_IN, F.OPERAND), 3, "the operand holds an abundance of 2^32 or more"),
    ]
    for idx, op_mh, rule, want_code, words in cases:
        pool, made = L.smh_pool_bytes(), count(pkg, "index_filtered")
        h, code, msg = raw(pkg, idx, op_mh, rule)
        assert h is None and code == want_code and words in msg, (msg, words)
        assert (code != 3) or msg.startswith("filter: "), msg
        assert L.smh_pool_bytes() == pool and count(pkg, "index_filtered") == made, words     # nothing built
        if idx is index:
            assert index.find(mk(pkg, [2]), 0.0) == [0, 1], words   # the parent still answers
    # what the abundances refuse, a rule that does not involve them takes
    check(pkg, wide, [[(1, 1)], [(1, 2), (5, 1 << 32)]], abund="flat", max_owners=1)
    check(pkg, wide, [[(1, 1)], [(1, 2), (5, 1 << 32)]], [(5, 7)], "keep", abund="operand")
    check(pkg, index, sk, [(2, 1 << 32), (9, 1)], "keep", op_mh=op_wide)             # OWN: the operand's abundances are not read
    # select: an id beyond the nodes names its position; NULL index; NULL ids
    u32p = C.POINTER(C.c_uint32)
    for handle, ids, k, words in ((index._h, [0, 2, 3], 3, "ids[2] is 3; the index has 3 nodes"), (None, [0], 1, "index is NULL"),
                                  (index._h, None, 2, "ids is NULL")):
        pool, made = L.smh_pool_bytes(), count(pkg, "index_selected")
        L.sourmash_err_clear()
        arr = np.array(ids, dtype=np.uint32) if ids is not None else None
        assert L.smh_index_select(handle, arr.ctypes.data_as(u32p) if arr is not None else None, k) is None
        with pytest.raises(pkg.SourmashError) as ei:
            pkg.errors.check()
        assert ei.value.code == 3 and ei.value.message.startswith("select: ") and words in ei.value.message
        assert L.smh_pool_bytes() == pool and count(pkg, "index_selected") == made


def test_work_space_returns_to_the_pool(pkg):
    L = pkg.lib()
    sketches, uni = layout(71, [500, 3000, 0, 20])
    index = index_of(pkg, sketches)
    op_mh = mk(pkg, [(h, 2) for h in uni[::2]])
    index.filter(max_owners=1)
    for kw in (dict(operand=op_mh, mode="keep", abund="operand"), dict(max_owners=1), dict(operand=op_mh, mode="drop", min_abund=2)):
        child = index.filter(**kw)
        child = None
        before = L.smh_pool_bytes()
        for _ in range(2):
            child = index.filter(**kw)
            assert len(child) == 4
            child = None
            assert L.smh_pool_bytes() == before, kw
