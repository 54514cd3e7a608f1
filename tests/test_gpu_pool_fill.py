"""What device work space holds before the library writes it must reach no result.  Every byte of device memory the library
uses comes from device_pool_alloc; smh_set_pool_fill makes it fill every block it hands out or parks with a byte.  Every
operation here runs four times -- under the bytes 0x00 (what new VRAM holds), 0x5A (a pattern that is no valid index, rank,
count or flag) and 0xFF (all ones: hash 2^64 - 1, rank 2^32 - 1, abundance 2^32 - 1), and with the fill off -- each time after
smh_release_workspace(), and each time it builds all its sketches, indexes, collections and trees anew, so that no block the
library owns escapes the fill.  The event counter "pool_filled" must rise under the three bytes and stand still with the fill
off.  Every expected value comes from a plain-Python restatement or the C oracle, never from a run of the library; all
outputs are integers or rule-defined doubles and are compared with `==` (angular similarity within the bound of
test_gpu_angular.py, NaN positions as test_gpu_compare_small_routes.py compares them).

Three kinds of test:
  * the families of operations at the smallest shapes that take their multi-workgroup paths (counters, scans and partial
    sums live in work space between kernels there); many of them are the bodies of tests of the other files, which read the
    tile and branch sizes from the *_geometry() calls;
  * planted pads: a CSR of S hashes is allocated with S * 8 + 8 bytes and more, and the compare kernels read a little past
    its end.  W64 = the fill byte eight times is then what they read: a set ends directly in front of the pad WITHOUT holding
    W64 while the other side of the comparison DOES hold it (hash 0 under 0x00, hash 2^64 - 1 under 0xFF).  A kernel that
    counted what it read there would count one hash too many;
  * children kept after their parents: a block that is given back is filled as well, so a child that kept a pointer into
    its parent's or an operand's memory reads the pattern."""
import ctypes as C
import gc
import random

import numpy as np
import pytest

import angular_restatement as AR
import cluster_restatement as CR
import collapse_restatement as CO
import downsample_restatement as DR
import filter_restatement as F
import gather_restatement as GR
import index_build_restatement as IB
import lca_restatement as LR
import match_restatement as MR
import pair_restatement as PR
import sbt_restatement as SBR
import search_many_restatement as SR
import test_gpu_angular as TA
import test_gpu_cluster as TC
import test_gpu_collapse as TCO
import test_gpu_compare as TCMP
import test_gpu_compare_small_routes as TSR
import test_gpu_downsample as TD
import test_gpu_fastx as TFX
import test_gpu_filter as TF
import test_gpu_gather as TG
import test_gpu_gather_many as TGM
import test_gpu_grid_trips as TGT
import test_gpu_index_build as TIB
import test_gpu_lca as TL
import test_gpu_match as TM
import test_gpu_sbt as TSBT
import test_gpu_search_many as TS
import test_gpu_sketch as TSK
import test_gpu_sort as TSO

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
U64 = np.uint64
FILLS = (0x00, 0x5A, 0xFF, -1)
ALL = TSR.ALL
mk, count = TG.mk, TG.count


def W64(p):
    """what eight bytes of the fill read as; with the fill off the tests plant the 0x5A pattern all the same"""
    return (p if p >= 0 else 0x5A) * 0x0101010101010101


def W32(p):
    return (p if p >= 0 else 0x5A) * 0x01010101


@pytest.fixture(autouse=True)
def off_between_tests(pkg):
    """the fill is off when a test begins -- the one before it, passed or failed, put it back -- and when it ends"""
    assert pkg.matrix.pool_fill() == -1 == pkg.lib().smh_pool_fill()
    yield
    assert pkg.matrix.pool_fill() == -1 == pkg.lib().smh_pool_fill()


@pytest.fixture
def fill(pkg):
    """sets the fill byte; the fill is off again when the test ends, however it ends"""
    try:
        yield pkg.matrix.set_pool_fill
    finally:
        pkg.matrix.set_pool_fill(-1)


def under_fills(pkg, fill, fn, resets=False):
    """fn(p) under every fill byte and with the fill off, each time behind smh_release_workspace(): "pool_filled" rises under
    the bytes and stands still without.  resets: fn calls smh_profile_reset, which zeroes the counter -- then the counter
    itself is read instead of its rise."""
    L = pkg.lib()
    for p in FILLS:
        gc.collect()
        assert L.smh_release_workspace() == 0 and L.smh_pool_bytes() == 0
        fill(p)
        assert pkg.matrix.pool_fill() == p
        before = 0 if resets else count(pkg, "pool_filled")
        fn(p)
        moved = count(pkg, "pool_filled") - before
        assert moved > 0 if p >= 0 else moved == 0, (p, moved)
    gc.collect()


# ---------------------------------------------------------------------------------- the knob and the work space

def test_release_gives_everything_back_and_every_new_block_is_filled(pkg, fill, coracle):
    """After smh_release_workspace() the pool holds nothing.  A scaled sketch of two batches then allocates the candidate
    buffers, the tile records (Device::tile_rec), the ring of tile counters and, for the second batch, the union's
    temporaries (Engine::union_tmp): under a byte each of them is a block that is filled, and the sketch is the oracle's."""
    L = pkg.lib()
    mx = M64 // 50
    parts = [bytes(coracle.synth_dna(0, 60000, 3, 0)), bytes(coracle.synth_dna(30000, 60000, 3, 0))]
    o = coracle.MinHash(0, 21, False, 42, mx, True)
    for part in parts:
        o.add_sequence(part, True)
    assert len(o.mins) > 1000 and max(o.abunds) > 1
    filled = {}

    def run(p):
        g = pkg.KmerMinHash(0, 21, False, 42, mx, True)
        first = count(pkg, "pool_filled")
        g.add_sequences([parts[0]], True)
        second = count(pkg, "pool_filled")
        g.add_sequences([parts[1]], True)
        filled[p] = (second - first, count(pkg, "pool_filled") - second)
        assert g.mins == o.mins and g.abunds == o.abunds, p
        g = None
        gc.collect()
        assert L.smh_release_workspace() == 0 and L.smh_pool_bytes() == 0

    under_fills(pkg, fill, run)
    for p in FILLS[:3]:
        assert filled[p][0] >= 4 and filled[p][1] >= 1, filled    # candidates, tile records, tile counters, scratch; the union
    assert filled[-1] == (0, 0) and filled[0x00] == filled[0x5A] == filled[0xFF]


# ---------------------------------------------------------------------------------- sketching, the sort, the parser

def test_dna_sketches(pkg, fill, coracle):
    """scaled with and without abundances, many batches into one sketch (fold + union on the device); bottom-num sketches
    longer than one chunk, with and without abundances"""
    def run(p):
        TSK.test_scaled_sketch_accumulates_in_hbm_small(False, True, pkg, coracle)
        TSK.test_scaled_sketch_accumulates_in_hbm_small(False, False, pkg, coracle)
        for num, k, track in ((50, 12, True), (2000, 21, False)):
            seq = bytes(coracle.synth_dna(0, 200000, 11 + num, 0))
            seq = seq[:80000] + seq[:50000] + seq[80000:]
            g, o = pkg.KmerMinHash(num, k, False, 42, 0, track), coracle.MinHash(num, k, False, 42, 0, track)
            for part in (seq, seq[1000:60000]):
                g.add_sequence(part, True); o.add_sequence(part, True)
                TSK.same_state(g, o)

    under_fills(pkg, fill, run, resets=True)


def test_protein_and_translated_sketches(pkg, fill, coracle):
    """the translated six-frame arm into one scaled sketch over many batches; the fused protein kernel; bottom-num protein"""
    def run(p):
        TSK.test_scaled_sketch_accumulates_in_hbm_small(True, True, pkg, coracle)
        seq = bytes(coracle.synth_dna(0, 120000, 5, 3000))
        for case in ((0, 27, True, 42, M64 // 20, True), (300, 21, True, 42, 0, True), (0, 30, True, 42, M64 // 20, False)):
            g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
            for part in (seq[:80000], seq[40000:]):
                g.add_sequence(part, True); o.add_sequence(part, True)
                TSK.same_state(g, o)

    under_fills(pkg, fill, run, resets=True)


@pytest.mark.parametrize("n", [2047, 2048, 2049, 16383, 16384, 16385])
def test_sort(pkg, fill, n):
    under_fills(pkg, fill, lambda p: TSO.test_sizes_around_one_tile_and_eight(pkg, n))


def test_fastx_parse_across_a_tile_edge(pkg, fill):
    T = pkg.lib().smh_records_tile_bytes()
    rng = random.Random(2)
    body = TFX.dna(rng, 2 * T + 40)
    texts = []
    for at in (T - 1, T, T + 1):
        texts.append((b">f\n" + body[:at - 4] + b"\n" + b">hdr " + body[:5] + b"\n" + body[7:44] + b"\n" + body[50:61] + b"\n>z\n" + body[70:79], "fasta"))
        texts.append((b">f\n" + body[:at - 3] + b"\r\n" + body[9:30] + b"\r\n>z\r\n" + body[40:45], "fasta"))
    recs = TFX.fastq_records(rng, 3 * T // 300)
    texts.append((TFX.fastq_text(recs), "auto"))
    texts.append((TFX.fastq_text(recs, b"\r\n", last_eol=False), "fastq"))

    def run(p):
        for text, fmt in texts:
            TFX.check(pkg, text, fmt, True)
            TFX.check(pkg, text, fmt, False)

    under_fills(pkg, fill, run)


# ---------------------------------------------------------------------------------- compare

@pytest.mark.parametrize("total,part", [(257, slice(0, 4)), (8193, slice(0, 2)), (39935, slice(0, 4))])
def test_compare_pair_path(pkg, fill, total, part):
    """k_pair_block<256>, k_pair_block<1024> and (num 0, la + lb > 32 768) k_pair_grid, whose partial sums meet in PairOut"""
    under_fills(pkg, fill, lambda p: TSR.test_pair_path(total, total < 32768, part, pkg), resets=True)


SMALL_ROUTES = {
    "wave-structures": lambda pkg: TSR.test_wave_route_on_every_structure(257, pkg),
    "wave-second-pair": TSR.test_wave_route_workgroups_take_a_second_pair,      # more pairs than workgroups
    "few-grid-stride": lambda pkg: TSR.test_few_route_counts_of_streamed_sketches(-1, pkg),   # more streamed sketches than one pass
    "few-early-exit": lambda pkg: TSR.test_few_route_early_exit_edges(1, pkg),
}


@pytest.mark.parametrize("case", sorted(SMALL_ROUTES))
def test_compare_wave_and_few_routes(pkg, fill, case):
    under_fills(pkg, fill, lambda p: SMALL_ROUTES[case](pkg))


@pytest.mark.parametrize("tune,expect", [pytest.param(*r.values, id=r.id) for r in TCMP.BLOCK_ROUTES
                                         if r.id in ("components", "tiled", "tiled-no-frequent-split", "tiled-no-range-masks")])
def test_compare_block_routes(pkg, fill, coracle, tune, expect):
    """83 x 131 ragged sketches with per-row nums: the dictionary (pooled sort, ranks, components, partition table, range
    masks) and the plan are built anew in filled work space under every byte"""
    under_fills(pkg, fill, lambda p: TCMP.test_tiled_block_edge_cases(tune, expect, pkg, coracle))


@pytest.mark.parametrize("tune", [dict(), dict(route="tiled"), dict(split_frequent=False)], ids=["auto", "tiled", "no-split"])
def test_compare_frequent_hash_split(pkg, fill, coracle, tune):
    under_fills(pkg, fill, lambda p: TCMP.test_frequent_hashes_are_set_aside_exactly(3, "spread", tune, pkg, coracle))


@pytest.mark.parametrize("masks", [True, False], ids=["masks-built", "masks-over-budget"])
def test_compare_range_masks(pkg, fill, coracle, masks):
    under_fills(pkg, fill, lambda p: TCMP._range_mask_corners(150, 4500 if masks else 8000, masks, pkg, coracle))


def test_compare_sharded_world_3(pkg, fill, coracle):
    """the dictionary built by three owners played in this process: slices, shares, the mirrored-block exchange"""
    import torch
    from sourmash_rust_amd import distributed as D
    from sourmash_rust_amd import synth
    n, num = 130, 300
    sigs = synth.family_signatures(0, n, num=num, n_families=7, pool=2 * num, private=num // 2, seed=17)
    sigs[::3, 0] = 1                                              # a hash held by a third of them: set aside as frequent
    ocommon, osize, ojac = coracle.compare_matrix([sigs[i] for i in range(n)], [sigs[i] for i in range(n)], num, 31, 0)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(num)

    def run(p):
        t = torch.from_numpy(sigs.view(np.int64)).cuda()
        for tune in (dict(), dict(route="tiled"), dict(route="components")):
            with pkg.matrix.tuning(**tune):
                outs = D.simulate_sharded(t, n, num, 3, want=("jaccard", "common", "size"))
            assert (torch.cat([o["jaccard"] for o in outs]).cpu().numpy() == ojac).all(), (p, tune)
            assert (torch.cat([o["common"] for o in outs]).cpu().numpy().view(U64) == ocommon).all(), (p, tune)
            assert (torch.cat([o["size"] for o in outs]).cpu().numpy().view(U64) == osize).all(), (p, tune)

    under_fills(pkg, fill, run)


# ---------------------------------------------------------------------------------- planted pads

BLOCK_TUNES = (dict(route="wave"), dict(route="few"), dict(route="components"), dict(route="tiled"),
               dict(route="tiled", range_masks=False), dict(route="tiled", split_frequent=False, visit_all_tiles=True, use_symmetry=False))


def planted(p, variant, seed=0, size=33):
    """(sets, others): `sets` are the nodes of the index under test -- its last node ends directly in front of the pad and
    does not hold W64 -- `others` the other side, where three sketches hold W64.  variant: "full", "last_empty" (the last
    node is empty: the node before it ends in front of the pad) or "lonely" (every node but one is empty)."""
    w = W64(p)
    rng = np.random.default_rng(900 + seed)
    pool = sorted({int(x) for x in rng.integers(1, M64, 400, dtype=U64)} - {w})
    pick = lambda k: sorted(int(x) for x in rng.choice(pool, k, replace=False))
    last = pick(size)
    sets = {"full": [pick(40), [], pick(70), last], "last_empty": [pick(40), pick(70), last, []], "lonely": [[], [], last, []]}[variant]
    assert all(w not in s for s in sets)
    others = [sorted(set(last) | {w}), [w], sorted(set(pick(50)) | {w}), pick(60), last[:size // 2], []]
    return sets, others


def arrays(sketches):
    return [np.array(sorted(s), dtype=U64) for s in sketches]


def probe(pkg, index, held, others, p, what, tunes=BLOCK_TUNES, queries=True):
    """`index` must hold the sets `held`.  Its content as read(); the N x M compare on every route, both ways round and
    against itself in one collection with `others`; gather with a query that holds W64."""
    off, h, _ = index.read()
    assert off.tolist() == np.cumsum([0] + [len(s) for s in held]).tolist() and h.tolist() == [x for s in held for x in s], (what, p)
    other = pkg.index.ResidentIndex([mk(pkg, s) for s in others])
    exp, exp_t = PR.matrix(arrays(held), arrays(others), 0), PR.matrix(arrays(others), arrays(held), 0)
    exp_self = PR.matrix(arrays(held), arrays(held), 0)
    for tune in tunes:
        with pkg.matrix.tuning(**tune):
            TSR._same(index.compare(other, want=ALL), exp, ALL, (what, p, tune))
            TSR._same(other.compare(index, want=ALL), exp_t, ALL, (what, p, tune, "transposed"))
            TSR._same(index.compare(index, want=ALL), exp_self, ALL, (what, p, tune, "itself"))
    if not queries:
        return
    w = W64(p)
    query = sorted({x for s in held for x in s[::2]} | {w} | set(others[3]))
    ab = {x: 1 + x % 5 for x in query}
    for abunds in (None, ab):
        res = index.gather(mk(pkg, query, abunds), threshold_bp=1, scaled=1, abund_stats=False)
        want = GR.gather(held, query, abunds)
        assert TG.as_dicts(res.rows) == want[0] and res.assigned.tolist() == want[1], (what, p)
    exp_q = PR.matrix(arrays(held), arrays([query]), 0)
    for cont in (False, True):
        col = exp_q["containment" if cont else "jaccard"][:, 0]
        assert index.find(mk(pkg, query), 0.0, cont) == [v for v in range(len(held)) if col[v] > 0.0], (what, p, cont)


@pytest.mark.parametrize("variant", ["full", "last_empty", "lonely"])
def test_pad_of_an_uploaded_index(pkg, fill, variant):
    def run(p):
        sets, others = planted(p, variant)
        probe(pkg, pkg.index.ResidentIndex([mk(pkg, s) for s in sets]), sets, others, p, variant)

    under_fills(pkg, fill, run)


@pytest.mark.parametrize("variant", ["full", "last_empty", "lonely"])
def test_pad_of_packed_sketches(pkg, fill, variant):
    """smh_compare_block on host sketches: Engine::pack_sketches uploads both sides into work space with the same pad"""
    def run(p):
        sets, others = planted(p, variant, seed=1)
        exp, exp_t = PR.matrix(arrays(sets), arrays(others), 0), PR.matrix(arrays(others), arrays(sets), 0)
        a, b = [mk(pkg, s) for s in sets], [mk(pkg, s) for s in others]
        for tune in BLOCK_TUNES:
            with pkg.matrix.tuning(**tune):
                TSR._same(pkg.matrix.compare_block(a, b, want=ALL), exp, ALL, (variant, p, tune))
                TSR._same(pkg.matrix.compare_block(b, a, want=ALL), exp_t, ALL, (variant, p, tune, "transposed"))

    under_fills(pkg, fill, run)


@pytest.mark.parametrize("size", [33, 4500, 20000])
def test_pad_of_the_pairwise_calls(pkg, fill, size):
    """the pairwise ABI calls read the sketches' device mirrors: k_pair_block<256> (la + lb <= 8 192), k_pair_block<1024> and,
    above 32 768 with num 0, k_pair_grid, whose waves add their counts into a PairOut that is zeroed in front of the launch.
    One side holds W64, the other ends in front of its pad without it."""
    def run(p):
        w = W64(p)
        rng = np.random.default_rng(size)
        pool = np.setdiff1d(np.unique(rng.integers(1, M64, 3 * size, dtype=U64)), np.array([w], dtype=U64))
        a = np.sort(rng.choice(pool, size, replace=False))
        b = np.union1d(rng.choice(a, size // 2, replace=False), rng.choice(pool, size // 2, replace=False))
        b = np.union1d(b, np.array([w], dtype=U64))
        assert {33: a.size + b.size <= 8192, 4500: 8192 < a.size + b.size <= 32768, 20000: a.size + b.size > 32768}[size]
        ga, gb, ge = mk(pkg, a), mk(pkg, b), mk(pkg, [])
        for (x, gx), (y, gy) in (((a, ga), (b, gb)), ((b, gb), (a, ga)), ((a[:0], ge), (b, gb)), ((b, gb), (a[:0], ge))):
            common, sz, cc, jac, cont = PR.pair(x, y, 0)
            assert gx.intersection_size(gy) == (common, sz) and gx.count_common(gy) == cc and gx.compare(gy) == jac, (p, x.size, y.size)
            got = gx.containment(gy)
            assert (got == cont) if x.size else (got != got), (p, x.size, y.size)

    under_fills(pkg, fill, run)


def test_pad_of_the_abundances(pkg, fill):
    """angular: pair, query against index, matrix unpruned and pruned.  The last node's last abundance is W32 itself -- a real
    abundance next to the pad of the u32 array -- and a sketch of the other side holds hash W64."""
    min_pairs = pkg.lib().smh_angular_prune_min_pairs()

    def run(p):
        w, a32 = W64(p), max(1, W32(p))
        rng = np.random.default_rng(31)
        pool = sorted({int(x) for x in rng.integers(1, M64, 600, dtype=U64)} - {w})
        rows = [TA.subset(rng, pool, k, 50) for k in (64, 0, 129, 33)]
        rows[-1][max(rows[-1])] = a32
        cols = [{**TA.subset(rng, pool, 80, 50), w: 7}, {w: a32}, {**rows[-1], w: 3}, TA.subset(rng, pool, 65, 50), {}]
        for variant in (rows, rows + [{}], [{}, {}, rows[-1], {}]):
            rindex, cindex = pkg.index.ResidentIndex([TA.mk(pkg, r) for r in variant]), pkg.index.ResidentIndex([TA.mk(pkg, c) for c in cols])
            TA.same(*TA.matrix(rindex, cindex), AR.block(variant, cols), "planted, %d rows, fill %d" % (len(variant), p))
            TA.same(*TA.matrix(cindex, rindex), AR.block(cols, variant), "planted, transposed")
            TA.same(*TA.matrix(rindex), AR.block(variant, variant, symmetric=True), "planted, itself")
            for c in cols[:4]:
                res = rindex.angular(TA.mk(pkg, c))
                TA.same(res.dot, res.cosine, res.angular, [m[0] for m in AR.block([c], variant)], "")
            ang, cos, dot, na, nb = TA.mk(pkg, variant[-2 if not variant[-1] else -1]).angular_parts(TA.mk(pkg, cols[2]))
            e = AR.pair(variant[-2 if not variant[-1] else -1], cols[2])
            assert (dot, na, nb) == e[:3] and np.float64(cos).view(U64) == np.float64(e[3]).view(U64) and abs(ang - e[4]) <= TA.ANG_TOL
        # the pruned route: enough pairs that the count_common matrix decides which pairs are walked
        k = int(np.ceil(np.sqrt(min_pairs))) + 1
        many = [TA.subset(rng, pool, 5 + v % 7, 9) for v in range(k - 1)] + [rows[-1]]
        mindex = pkg.index.ResidentIndex([TA.mk(pkg, r) for r in many])
        TA.same(*TA.matrix(mindex), AR.block(many, many, symmetric=True), "pruned, itself")
        wide = cols + [TA.subset(rng, pool, 4, 9) for _ in range(k - len(cols))]
        TA.same(*TA.matrix(mindex, pkg.index.ResidentIndex([TA.mk(pkg, c) for c in wide])), AR.block(many, wide), "pruned, two indexes")

    under_fills(pkg, fill, run)


def weighted(sets, p):
    """abundances 1 .. 5, and W32 on the last hash in front of the pad"""
    out = [[(x, 1 + (x + v) % 5) for x in s] for v, s in enumerate(sets)]
    last = max(v for v, s in enumerate(sets) if s)
    out[last][-1] = (out[last][-1][0], max(1, W32(p)))
    return out


def test_pads_of_the_children(pkg, fill):
    """filter, select, cut, collapse and concat write a child whose last node ends in front of a pad nobody writes"""
    def run(p):
        w = W64(p)
        for variant in ("full", "last_empty", "lonely"):
            sets, others = planted(p, variant, seed=2)
            ws = weighted(sets, p)
            junk = sorted({3, 5, M64 - 9} - {w})
            # filter: the parent holds junk hashes (and, in a node of its own at the end, W64) that the operand removes
            parent_sets = [sorted(set(s) | set(junk)) if s else [] for s in sets] + [[w]]
            parent = pkg.index.ResidentIndex([mk(pkg, s) for s in parent_sets])
            child = parent.subtract(mk(pkg, junk + [w]))
            probe(pkg, child, sets + [[]], others, p, ("subtract", variant))
            kept = parent.intersect(mk(pkg, sorted({x for s in sets for x in s})))
            probe(pkg, kept, sets + [[]], others, p, ("intersect", variant), tunes=BLOCK_TUNES[2:4])
            # inflate: the operand's abundances, W32 among them, land next to the child's abundance pad
            flat_parent = pkg.index.ResidentIndex([mk(pkg, s) for s in sets])
            operand = sorted({x: a for s in ws for x, a in s}.items())
            inflated = flat_parent.inflate(TF.mk(pkg, operand))
            TF.same(inflated, F.filter(sets, operand, TF.rule_of("keep", "operand"), has_abunds=False, operand_tracks=True), ("inflate", variant, p))
            # select: the pad follows whatever node is picked last
            order = [v for v, s in enumerate(sets) if not s] + [v for v, s in enumerate(sets) if s]
            whole = pkg.index.ResidentIndex([mk(pkg, s) for s in sets + [[w], others[2]]])
            probe(pkg, whole.select(order), [sets[v] for v in order], others, p, ("select", variant), tunes=BLOCK_TUNES[:4])
            # cut: hashes above the new max_hash go, W64 with them under 0xFF
            half = 1 << 63
            low = [[x for x in s if x <= half] for s in sets]
            cut = pkg.index.ResidentIndex([mk(pkg, s) for s in sets]).downsample(max_hash=half)
            low_others = [[x for x in s if x <= half] for s in others]
            off, h, _ = cut.read()
            assert off.tolist() == np.cumsum([0] + [len(s) for s in low]).tolist() and h.tolist() == [x for s in low for x in s]
            cother = pkg.index.ResidentIndex([mk(pkg, s, max_hash=half) for s in low_others])
            for tune in BLOCK_TUNES[:4]:
                with pkg.matrix.tuning(**tune):
                    TSR._same(cut.compare(cother, want=ALL), PR.matrix(arrays(low), arrays(low_others), 0), ALL, ("cut", variant, p, tune))
            # collapse: groups in the nodes' order, so that the last group ends in front of the pad
            grouped = pkg.index.ResidentIndex([mk(pkg, s) for s in sets + [sets[0]]])
            group = [0, 1, 1, 2, 0] if variant != "last_empty" else [0, 1, 2, 3, 0]
            G = max(group) + 1
            united = grouped.collapse(group, G)
            want = CO.collapse(sets + [sets[0]], group, G)
            TCO.same(united, want, ("collapse", variant, p))
            probe(pkg, united, CO.sketches_of(*want[:2]), others, p, ("collapse", variant), tunes=BLOCK_TUNES[2:4])
            # concat: the last part's last node
            parts = [pkg.index.ResidentIndex([mk(pkg, s) for s in part]) for part in ([[w], others[2]], sets[:2], sets[2:])]
            probe(pkg, pkg.index.ResidentIndex.concat(parts), [[w], others[2]] + sets, others, p, ("concat", variant), tunes=BLOCK_TUNES[:4])

    under_fills(pkg, fill, run)


# ---------------------------------------------------------------------------------- angular, downsample

def test_angular(pkg, fill):
    """every row size against every column size (unpruned), a device-built query, and the pruned symmetric matrix"""
    min_pairs = pkg.lib().smh_angular_prune_min_pairs()
    rng = np.random.default_rng(21)
    pool = sorted({0, M64} | set(int(x) for x in rng.integers(1, M64, 12_000, dtype=U64)))
    rows = [TA.subset(rng, pool, k) for k in TA.ROW_SIZES]
    cols = [TA.subset(rng, pool, TA.COL_SIZES[j % len(TA.COL_SIZES)]) for j in range(13)]
    k = int(np.ceil(np.sqrt(2 * min_pairs))) + 2
    fam = [TA.subset(rng, pool[:900], 20 + v % 50, 30) for v in range(k)]
    exp, exp_fam = AR.block(rows, cols), AR.block(fam, fam, symmetric=True)

    def run(p):
        rindex, cindex = pkg.index.ResidentIndex([TA.mk(pkg, r) for r in rows]), pkg.index.ResidentIndex([TA.mk(pkg, c) for c in cols])
        TA.same(*TA.matrix(rindex, cindex), exp, "rows x 13 columns, fill %d" % p)
        assert pkg.matrix.angular_last_stats()[0] == sum(1 for r in rows if r) * sum(1 for c in cols if c)
        TA.same(*TA.matrix(pkg.index.ResidentIndex([TA.mk(pkg, s) for s in fam])), exp_fam, "pruned, fill %d" % p)
        walked, skipped = pkg.matrix.angular_last_stats()
        assert skipped > 0 and walked + skipped == k * (k - 1) // 2
        TA.test_query_built_on_the_device(pkg)

    under_fills(pkg, fill, run, resets=True)


def test_downsample(pkg, fill, coracle):
    """the block cut around its tile ends, a device-resident sketch (run starts and counts), an index cut in HBM"""
    T = pkg.matrix.downsample_geometry()[0]
    rng = np.random.default_rng(8)
    top = 1 << 60
    pool = np.unique(rng.integers(1, top, 3000, dtype=U64))
    fam = TD.family(rng, pool, 12, 400) + [([], [])] + TD.family(rng, pool, 3, 5)

    def run(p):
        for with_abunds in (False, True):
            TD.test_block_segment_ends_around_tile_ends(pkg, T, with_abunds, False)
        TD.test_device_sketch_cut(pkg, coracle, True, 2)
        TD.test_device_sketch_cut(pkg, coracle, False, 1)
        for moved in (False, True):
            parent = pkg.index.ResidentIndex([TD.mk(pkg, m, a, top) for m, a in fam])
            if moved:
                parent.norms2()                                   # the abundances live in HBM: the copy kernel cuts them
            child = parent.downsample(max_hash=top // 3)
            want = [DR.cut(m, a, top // 3) for m, a in fam]
            off, h, ab = child.read()
            assert off.tolist() == np.cumsum([0] + [len(m) for m, _ in want]).tolist(), (p, moved)
            assert h.tolist() == [x for m, _ in want for x in m] and ab.tolist() == [x for _, a in want for x in a], (p, moved)
            S = [dict(zip(m, a)) for m, a in want]
            TA.same(*TA.matrix(child), AR.block(S, S, symmetric=True), "cut index, fill %d" % p)

    under_fills(pkg, fill, run)


# ---------------------------------------------------------------------------------- SBT

def test_sbt_build_find_and_find_many(pkg, fill):
    d, n, sizes = 2, 150, [1009, 1013, 1019]
    thresholds = (0, 0.1, 0.3)
    cache = {}

    def run(p):
        rng = random.Random(2150)
        leaves = TSBT.family_leaves(pkg, rng, n, False, families=8)
        leaves[5] = pkg.KmerMinHash(300, 21, False, 42, 0, False)
        positions = pkg.sbt.default_positions(n, d)
        t = pkg.SBT.build(leaves, sizes, ksize=21, d=d, positions=positions)
        queries = [leaves[i] for i in range(0, n, 7)] + [leaves[5]]
        if not cache:                                             # the restatement, once: the leaves are the same every time
            nodes, lv = TSBT.restated(d, sizes, positions, leaves, lambda mh: mh.num)
            cache["want"] = {(thr, cont): [SBR.find(d, sizes, nodes, lv, list(q.mins), thr, cont) for q in queries]
                             for thr in thresholds for cont in (False, True)}
            assert sum(map(len, cache["want"][(0.1, False)])) > len(queries)
        for (thr, cont), want in cache["want"].items():
            assert t.find_many(queries, thr, cont) == want, (p, thr, cont)
            for q, hits in list(zip(queries, want))[::5]:
                assert t.find_positions(q, thr, cont) == hits, (p, thr, cont)

    under_fills(pkg, fill, run)


# ---------------------------------------------------------------------------------- gather and the batched queries

@pytest.fixture(scope="module")
def nodes(pkg):
    return TGT.Nodes(29, pkg.matrix.search_geometry()[0])


@pytest.fixture(scope="module")
def batch(nodes):
    return TGT.Batch(nodes)


def test_gather(pkg, fill, nodes):
    """abundances as none, as host pairs, as u64 counts in HBM and as the run starts of a bulk fold"""
    exp = {w: GR.gather(nodes.sketches, nodes.query, nodes.ab if w else None) for w in (True, False)}
    assert len(exp[True][0]) >= 5

    def run(p):
        index = nodes.index(pkg)
        starts = pkg.KmerMinHash(0, 21, False, 42, M64, True)
        starts.add_many(np.repeat(np.array(nodes.query, dtype=U64), [nodes.ab[h] for h in nodes.query]))
        counts = mk(pkg, nodes.query, nodes.ab)
        assert counts.export_dev() == len(nodes.query)
        for q, w in ((mk(pkg, nodes.query), False), (mk(pkg, nodes.query, nodes.ab), True), (counts, True), (starts, True)):
            res = index.gather(q, threshold_bp=1, scaled=1, abund_stats=False)
            assert TG.as_dicts(res.rows) == exp[w][0] and res.assigned.tolist() == exp[w][1], (p, w)

    under_fills(pkg, fill, run)


def test_gather_many(pkg, fill, nodes, batch):
    exp = {w: [GR.gather(nodes.sketches, q, a if w else None) for q, a in zip(batch.queries, batch.abunds)] for w in (True, False)}

    def run(p):
        index = nodes.index(pkg)
        flat = [mk(pkg, q) for q in batch.queries]
        heavy = [mk(pkg, q, a) for q, a in zip(batch.queries, batch.abunds)]
        assert heavy[0].export_dev() == 150
        q3, a3 = batch.queries[3], batch.abunds[3]
        heavy[3] = pkg.KmerMinHash(0, 21, False, 42, M64, True)
        heavy[3].add_many(np.repeat(np.array(q3, dtype=U64), [a3[h] for h in q3]))
        for qs, w in ((flat, False), (heavy, True)):
            res = index.gather_many(qs, threshold_bp=1, scaled=1, abund_stats=False)
            assert [(TGM.as_dicts(r.rows), r.assigned.tolist()) for r in res] == exp[w], (p, w)

    under_fills(pkg, fill, run)


@pytest.mark.parametrize("metric", SR.METRICS)
def test_search_many_and_search_self(pkg, fill, nodes, batch, metric):
    shared, own = SR.shared(nodes.sketches, batch.queries), SR.shared(nodes.sketches, nodes.sketches)
    thresholds = (0.0, 0.04)
    exp = [SR.select(shared, metric, t) for t in thresholds]
    exp_self = {(t, up): [[r for r in rows if (r[0] > q if up else r[0] != q)] for q, rows in enumerate(SR.select(own, metric, t))]
                for t in thresholds for up in (True, False)}

    def run(p):
        index = nodes.index(pkg)
        qs = [mk(pkg, q) for q in batch.queries]
        for t, want in zip(thresholds, exp):
            assert TS.per_query(index.search_many(qs, t, TS.NAMES[metric], scaled=1)) == want, (p, t)
        for (t, up), want in exp_self.items():
            assert TS.per_query(index.pairwise(t, TS.NAMES[metric], upper=up)) == want, (p, t, up)

    under_fills(pkg, fill, run)


# ---------------------------------------------------------------------------------- cluster, match, lca

@pytest.mark.parametrize("metric", [CR.JACCARD, CR.MAX_CONTAINMENT])
def test_cluster(pkg, fill, metric):
    """600 nodes, two hubs with adjacency lists longer than kClusterLaneMax, chains that take several rounds: both linkages"""
    n = 600
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
    exp = {link: CR.cluster(sketches, metric, 0.0, 0, link, scores) for link in (CR.COMPONENTS, CR.GREEDY)}
    assert 3 < exp[CR.COMPONENTS][3] < exp[CR.GREEDY][3] < n

    def run(p):
        index = pkg.index.ResidentIndex([mk(pkg, s) for s in sketches])
        for link in (CR.COMPONENTS, CR.GREEDY):
            assert TC.as_lists(index.cluster(0.0, TC.NAMES[metric], TC.LINKS[link], scores=scores, scaled=1)) == exp[link], (p, link)

    under_fills(pkg, fill, run)


@pytest.fixture(scope="module")
def reads(pkg, pyoracle):
    return TGT.Reads(pyoracle, pkg.matrix.match_geometry()[0], pkg.matrix.lca_geometry()[1])


def test_match_with_hit_list(pkg, fill, reads):
    """rows (the four sums of a MatchRow) and hit lists: the LDS tally, the dense record, a record without hits or windows"""
    owners = MR.owners_of(reads.nodes)
    exp = {name: MR.match(recs, 21, 42, M64, owners) for name, recs in (("long", reads.records), ("short", reads.short))}

    def run(p):
        index = TM.make_index(pkg, reads.nodes)
        for name, recs in (("long", reads.records), ("short", reads.short)):
            res = index.match(recs, hits=True)
            assert TM.rows_of(res) == exp[name][0], (p, name)
            assert res.hit_offsets.tolist() == exp[name][1] and res.hit_hashes.tolist() == exp[name][2], (p, name)
            assert TM.rows_of(index.match(recs)) == exp[name][0], (p, name)

    under_fills(pkg, fill, run)


def test_lca_records(pkg, fill, reads):
    owners = MR.owners_of(reads.nodes)
    exp = {name: LR.classify_records(reads.parent, reads.node_taxon, owners, recs, 21, 42, M64)
           for name, recs in (("long", reads.records), ("short", reads.short))}

    def run(p):
        index = TL.make_index(pkg, reads.nodes, reads.parent, reads.node_taxon)
        for name, recs in (("long", reads.records), ("short", reads.short)):
            assert TL.rows_of(index.lca_classify_records(recs)) == exp[name], (p, name)

    under_fills(pkg, fill, run)


def test_lca_counts(pkg, fill):
    """a directory of 700 ranks over 30 nodes, every fifth with more than kLcaOwnerLaneMax owners; 5 queries, one empty"""
    lane = pkg.matrix.lca_geometry()[0]
    rng = random.Random(31)
    parent = TL.bushy(rng, 200)
    n = 30
    node_taxon = [rng.randrange(len(parent)) if v % 6 else TL.NO for v in range(n)]
    hashes = TL.unrelated(rng, 700)
    lengths = [1, 2, lane, lane + 1, 3, 1, lane + 4, 2, 1, 2 * lane + 3]
    held = [[] for _ in range(n)]
    for k, h in enumerate(hashes):
        for v in rng.sample(range(n), lengths[k % 10]):
            held[v].append(h)
    foreign = TL.unrelated(random.Random(32), 60)
    queries = [rng.sample(hashes, 150), [], rng.sample(hashes, 130) + foreign[:30], rng.sample(hashes, 283), rng.sample(hashes, 101) + foreign[30:]]
    owners = LR.owners_of(held)
    exp = [LR.counts(parent, node_taxon, owners, q) for q in queries]
    assert len(exp[0][0]) > 3 and exp[1] == ([], [])

    def run(p):
        index = TL.make_index(pkg, held, parent, node_taxon)
        got = index.lca_counts([TL.sketch(pkg, q) for q in queries], hash_taxon=True)
        for k, ((taxa, cnt, per), (pairs, want_per)) in enumerate(zip(got, exp)):
            assert per.tolist() == want_per and list(zip(taxa.tolist(), cnt.tolist())) == pairs, (p, k)

    under_fills(pkg, fill, run)


# ---------------------------------------------------------------------------------- collapse, index build, concat, filter, select

@pytest.fixture(scope="module")
def owned(pkg):
    lane_max, wave_max, _ = pkg.matrix.collapse_geometry()
    return TGT.Owned(lane_max, wave_max)


@pytest.mark.parametrize("abund", ["flat", "sum", "count"])
def test_collapse(pkg, fill, owned, abund):
    """union, core and prevalence; owner lists in the lane, wave and workgroup regimes; groups over more than two group tiles"""
    tile = pkg.matrix.collapse_geometry()[2]
    n, G = owned.n, 2 * tile + 5
    cases = [([(v // 2) * 27 + 75 for v in range(n)], G, 2, 0.0), ([None if v % 9 == 4 else v % 7 for v in range(n)], 7, 20, 0.0),
             ([0] * n, 1, 1, 0.5)]
    assert max(cases[0][0]) < G
    src = owned.sketches if abund == "sum" else TCO.flat(owned.sketches)
    exp = [CO.collapse(src, group, g, mc, mf, TCO.MODES[abund]) for group, g, mc, mf in cases]

    def run(p):
        index = TCO.index_of(pkg, owned.sketches)
        for (group, g, mc, mf), want in zip(cases, exp):
            TCO.same(index.collapse(group, g, mc, mf, abund), want, "fill %d G=%d" % (p, g))

    under_fills(pkg, fill, run)


def test_index_build_and_concat(pkg, fill):
    rng = np.random.default_rng(41)
    lens = [70, 90, 20, 64, 85, 40, 33, 120, 41, 75, 21, 60, 95, 226]
    records = [TIB.dna(rng, n) for n in lens]
    records[7] = records[1][:60] + records[7][60:]
    groups = [3, 0, 1, 4, 2, 1, 5, 0, 6, 3, 7, 8, 0, 10]
    many = [TIB.dna(rng, 21 + k % 4) for k in range(600)]
    prm = TIB.params(TIB.like_of(pkg, 21))
    exp, exp_many = IB.build(records, groups, 11, prm), IB.build(many, None, 600, prm)
    exp_joined = IB.concat([exp_many, exp, exp_many])

    def run(p):
        R, like = pkg.index.ResidentIndex, TIB.like_of(pkg, 21)
        built = R.from_records(records, like, groups, 11)
        assert TIB.triple(built) == exp, p
        lots = R.from_records(many, like)
        assert TIB.triple(lots) == exp_many, p
        assert TIB.triple(R.concat([lots, built, lots])) == exp_joined, p

    under_fills(pkg, fill, run)


def test_filter_and_select(pkg, fill):
    """operand, abundance and owner windows and inflate over nodes that cross tiles; select with repeats"""
    T = pkg.matrix.filter_geometry()[0]
    sketches, uni = TF.layout(51, [T + 3, 0, 2 * T + 1, 70, T])
    operand = [(h, 1 + h % 9) for h in uni[::2]]
    picks = [[4, 2, 2, 0, 1, 3], [3], []]

    def run(p):
        index, op_mh = TF.index_of(pkg, sketches), TF.mk(pkg, operand)
        TF.check(pkg, index, sketches, operand, "keep", op_mh=op_mh, abund="operand")
        TF.check(pkg, index, sketches, operand, "drop", op_mh=op_mh, min_abund=2, max_owners=1)
        TF.check(pkg, index, sketches, operand, "keep", op_mh=op_mh)
        TF.check(pkg, index, sketches, min_owners=2, abund="flat")
        TF.check(pkg, index, sketches, min_abund=2, max_abund=4)
        for moved in (False, True):
            if moved:
                index.angular_matrix()
            for ids in picks:
                TF.same(index.select(ids), F.select(sketches, ids), (p, ids))

    under_fills(pkg, fill, run)


# ---------------------------------------------------------------------------------- children kept after their parents

def test_children_outlive_their_parents(pkg, fill):
    """filter, select, downsample, collapse and concat: the child is built, the parent and every operand are deleted (their
    blocks are parked -- and filled), an unrelated index of similar size takes the parked blocks, and only then the child is
    read and queried.  A pointer kept into a parent's memory reads the pattern or the stranger's hashes."""
    rng = np.random.default_rng(77)
    uni = sorted({int(x) for x in rng.integers(1, M64, 4000, dtype=U64)})
    sets = [[(int(h), 1 + int(h) % 6) for h in sorted(rng.choice(uni, k, replace=False).tolist())] for k in (700, 0, 900, 64, 333)]
    flat = TF.flat(sets)
    operand = [(h, 2 + h % 3) for h in uni[::2]]
    half = 1 << 63
    group = [0, 1, 1, 2, 0]
    makers = {
        "filter": (lambda i, op: i.filter(op, "keep", abund="operand"), F.filter(sets, operand, TF.rule_of("keep", "operand"), has_abunds=True, operand_tracks=True)),
        "owners": (lambda i, op: i.filter(max_owners=1), F.filter(sets, None, TF.rule_of(max_owners=1), has_abunds=True, operand_tracks=True)),
        "select": (lambda i, op: i.select([4, 2, 2, 0]), F.select(sets, [4, 2, 2, 0])),
        "downsample": (lambda i, op: i.downsample(max_hash=half), None),
        "collapse": (lambda i, op: i.collapse(group, 3, abund="sum"), CO.collapse(sets, group, 3, 1, 0.0, CO.SUM)),
        "concat": (lambda i, op: pkg.index.ResidentIndex.concat([i, TF.index_of(pkg, sets[:2]), i]), None),
    }
    cut = [[(h, a) for h, a in s if h <= half] for s in sets]
    csr = lambda ss: (np.cumsum([0] + [len(s) for s in ss]).tolist(), [h for s in ss for h, _ in s], [a for s in ss for _, a in s])
    wants = {k: v[1] for k, v in makers.items()}
    wants["downsample"], wants["concat"] = csr(cut), csr(sets + sets[:2] + sets)

    def run(p):
        for name, (make, _) in makers.items():
            parent, op_mh = TF.index_of(pkg, sets), TF.mk(pkg, operand)
            parent.norms2()                                       # the abundances live in HBM: the children copy them there
            child = make(parent, op_mh)
            if name == "downsample":
                parent.drop_downsampled()                         # (the parent keeps its cuts; the child is ours alone now)
            del parent, op_mh
            gc.collect()
            stranger = TF.index_of(pkg, [[(h ^ 0x5555, 7) for h, _ in s] for s in sets])
            stranger.norms2()
            want = wants[name]
            TF.same(child, want, (name, p))
            held = CO.sketches_of(*want)
            mx = half if name == "downsample" else M64
            query = sorted(h for h in {h for s in held for h, _ in s[::3]} | set(uni[1::50]) if h <= mx)
            ab = {h: 1 + h % 4 for h in query}
            res = child.gather(mk(pkg, query, ab, max_hash=mx), threshold_bp=1, scaled=1, abund_stats=False)
            exp = GR.gather(TF.flat(held), query, ab)
            assert TG.as_dicts(res.rows) == exp[0] and res.assigned.tolist() == exp[1], (name, p)
            S = [dict(s) for s in held]
            TA.same(*TA.matrix(child), AR.block(S, S, symmetric=True), "%s kept after its parent, fill %d" % (name, p))
            del stranger, child
            gc.collect()

    under_fills(pkg, fill, run)
