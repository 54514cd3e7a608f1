"""Taxonomic LCA on a resident index on the device against tests/lca_restatement.py: everything must be
EQUAL.  The shapes stand on both sides of the sizes smh_lca_geometry and smh_match_geometry report (owner lists one lane or
one wave folds, records one lane or one wave folds, the probe's LDS sample).  A second witness -- match(hits=True) and the
literal rule on the hit hashes it returns -- is near the end."""
import ctypes as C
import random

import numpy as np
import pytest

import lca_restatement as R
import match_restatement as M

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
NO = R.NO_TAXON
FIELDS = ("windows", "distinct", "hit_distinct", "assigned_distinct", "taxon", "status")


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


def sketch(pkg, hashes, ksize=21, max_hash=M64):
    mh = pkg.KmerMinHash(0, ksize, False, 42, max_hash)
    if len(hashes):
        mh.add_many(np.array(sorted(hashes), dtype=np.uint64))
    return mh


def make_index(pkg, nodes, parent, node_taxon, ksize=21, max_hash=M64):
    index = pkg.index.ResidentIndex([sketch(pkg, n, ksize, max_hash) for n in nodes])
    index.set_taxonomy(parent, node_taxon)
    return index


def chain(n):
    return [0] + list(range(n - 1))


def bushy(rng, n):
    return [0] + [rng.randrange(max(0, t - 40), t) for t in range(1, n)]


def unrelated(rng, n):
    out = set()
    while len(out) < n:
        out.add(rng.getrandbits(64) | 1)
    return sorted(out)


def check_counts(pkg, index, parent, node_taxon, nodes, queries, max_hash=M64, sketches=None):
    """lca_counts with the per-hash taxa next to the restatement's; returns the library's answer"""
    owners = nodes if isinstance(nodes, dict) else R.owners_of(nodes)
    got = index.lca_counts(sketches or [sketch(pkg, q, max_hash=max_hash) for q in queries], hash_taxon=True)
    assert len(got) == len(queries)
    for q, (taxa, cnt, per) in zip(queries, got):
        want_pairs, want_per = R.counts(parent, node_taxon, owners, [h for h in q if h <= max_hash])
        assert per.tolist() == want_per
        assert list(zip(taxa.tolist(), cnt.tolist())) == want_pairs
        assert taxa.dtype == np.uint32 and cnt.dtype == np.uint64
    plain = index.lca_counts(sketches or [sketch(pkg, q, max_hash=max_hash) for q in queries])
    for (t0, c0), (t1, c1, _) in zip(plain, got):
        assert np.array_equal(t0, t1) and np.array_equal(c0, c1)
    return got


def rows_of(res):
    return list(zip(*[[int(x) for x in getattr(res, f)] for f in FIELDS]))


def check_records(pkg, index, parent, node_taxon, nodes, records, ksize=21, max_hash=M64):
    owners = nodes if isinstance(nodes, dict) else R.owners_of(nodes)
    want = R.classify_records(parent, node_taxon, owners, records, ksize, 42, max_hash)
    res = index.lca_classify_records(records)
    got = rows_of(res)
    assert len(got) == len(want)
    bad = [i for i in range(len(got)) if got[i] != want[i]]
    assert not bad, (bad[:5], [got[i] for i in bad[:5]], [want[i] for i in bad[:5]])
    m = index.match(records)
    for f in ("windows", "distinct", "hit_distinct"):
        assert np.array_equal(getattr(res, f), getattr(m, f)), f
    return got


@pytest.fixture(scope="module")
def geometry(pkg):
    owner_lane_max, record_lane_max, threads = pkg.matrix.lca_geometry()
    assert 2 <= owner_lane_max < 62 and 2 <= record_lane_max < 62 and threads == 64
    return owner_lane_max, record_lane_max, pkg.matrix.match_geometry()[2]


@pytest.fixture(scope="module")
def genome(pyoracle):
    return pyoracle.synth_dna(0, 6000, 21)


# ---------------------------------------------------------------------------------- the table

@pytest.fixture(scope="module")
def wide(pkg, geometry):
    """3 000 nodes over a bushy 1 000-taxon tree; hash k is held by the first sizes[k] nodes of a shuffled order"""
    rng = random.Random(11)
    lane = geometry[0]
    sizes = [1, 2, lane - 1, lane, lane + 1, 63, 64, 65, 129, 3000, 1, lane + 1, 64]
    parent = bushy(rng, 1000)
    node_taxon = [rng.randrange(1000) if rng.random() < 0.9 else NO for _ in range(3000)]
    nodes = [[] for _ in range(3000)]
    hashes = unrelated(rng, len(sizes) + 3)
    for k, size in enumerate(sizes):
        for node in rng.sample(range(3000), size):
            nodes[node].append(hashes[k])
    lonely = [i for i in range(3000) if node_taxon[i] == NO]
    for node in lonely[:lane + 3]:
        nodes[node].append(hashes[-3])            # a long list whose owners all have no lineage
    nodes[lonely[0]].append(hashes[-2])           # a short one
    return parent, node_taxon, nodes, hashes, make_index(pkg, nodes, parent, node_taxon)


def test_owner_lists_around_the_lane_limit_and_the_wave(pkg, wide):
    parent, node_taxon, nodes, hashes, index = wide
    built = count(pkg, "lca_table_built")
    got = check_counts(pkg, index, parent, node_taxon, nodes, [hashes, hashes[:3], [hashes[-1]]])
    per = got[0][2].tolist()
    assert per[hashes.index(hashes[-3])] == NO and per[-2] == NO and per[-1] == NO, "owners without a lineage assign nothing"
    # (three hashes are unassigned by construction; the three lists of one or two owners may fall on nodes without a lineage)
    assert sum(1 for t in per if t != NO) >= len(hashes) - 6
    assert count(pkg, "lca_table_built") == built + 1


@pytest.mark.parametrize("shape", ["depth1", "chain40", "root_only"])
def test_taxonomy_shapes(pkg, geometry, shape):
    rng = random.Random(3)
    lane = geometry[0]
    parent = {"depth1": [0] * 30, "chain40": chain(41), "root_only": [0]}[shape]
    n_taxa = len(parent)
    node_taxon = [rng.randrange(n_taxa) for _ in range(100)] + [NO] * 4
    hashes = unrelated(rng, 60)
    nodes = [[] for _ in range(104)]
    for k, h in enumerate(hashes):
        for node in rng.sample(range(104), [1, 2, lane, lane + 1, 70][k % 5]):
            nodes[node].append(h)
    index = make_index(pkg, nodes, parent, node_taxon)
    got = check_counts(pkg, index, parent, node_taxon, nodes, [hashes, hashes[::2], []])
    if shape == "chain40":
        assert len(set(got[0][0].tolist())) > 5


def test_all_owners_without_a_lineage(pkg):
    hashes = unrelated(random.Random(4), 20)
    nodes = [hashes[:12], hashes[5:], hashes[::3]]
    index = make_index(pkg, nodes, [0, 0, 1], [NO, NO, NO])
    got = check_counts(pkg, index, [0, 0, 1], [NO, NO, NO], nodes, [hashes])
    assert got[0][0].size == 0 and set(got[0][2].tolist()) == {NO}
    rows = index.lca_classify_records([b"ACGT" * 20])
    assert rows.taxon.tolist() == [NO] and rows.status.tolist() == [0]


# ---------------------------------------------------------------------------------- the directory

@pytest.mark.parametrize("delta", [-1, 0, 1, "x4"])
def test_directory_around_the_lds_sample(pkg, geometry, delta):
    samples = geometry[2]
    size = 4 * samples + 3 if delta == "x4" else samples + delta
    rng = random.Random(size)
    everything = unrelated(rng, size + 2)
    below, above, resident = everything[0], everything[-1], everything[1:-1]
    parent = bushy(rng, 50)
    node_taxon = [7, 19, NO, 33]
    nodes = [resident[0::3], resident[1::3], resident[2::3] + resident[:50], resident[::97]]
    index = make_index(pkg, nodes, parent, node_taxon)
    q0 = [below, resident[0], resident[1], resident[size // 2], resident[-2], resident[-1], above]
    got = check_counts(pkg, index, parent, node_taxon, nodes, [q0, resident[::5] + unrelated(random.Random(1), 100), [below], [above]])
    assert got[0][2][0] == NO and got[0][2][-1] == NO and got[2][0].size == 0 and got[3][0].size == 0


# ---------------------------------------------------------------------------------- the sketch route

@pytest.fixture(scope="module")
def small(pkg):
    rng = random.Random(21)
    parent = bushy(rng, 200)
    node_taxon = [rng.randrange(200) if i % 7 else NO for i in range(40)]
    pool = unrelated(rng, 3000)
    nodes = [rng.sample(pool, rng.choice([0, 5, 200, 900])) for _ in range(40)]
    queries = [rng.sample(pool, 300), [], unrelated(random.Random(99), 50), rng.sample(pool, 1200), rng.sample(pool, 7)]
    queries.append(list(queries[0]))              # the same query twice
    return parent, node_taxon, nodes, queries, make_index(pkg, nodes, parent, node_taxon)


def test_empty_disjoint_and_repeated_queries(pkg, small):
    parent, node_taxon, nodes, queries, index = small
    got = check_counts(pkg, index, parent, node_taxon, nodes, queries)
    assert got[1][0].size == 0 and got[2][0].size == 0 and got[0][0].size > 3
    assert np.array_equal(got[0][0], got[5][0]) and np.array_equal(got[0][1], got[5][1])
    assert index.lca_counts([]) == []
    # the host helpers on the small output
    taxa, cnt, _ = got[3]
    want_pairs, _ = R.counts(parent, node_taxon, R.owners_of(nodes), queries[3])
    assert pkg.index.lca_summarize(parent, taxa, cnt) == R.rollup(parent, want_pairs)
    for thr in (1, 3):
        assert pkg.index.lca_classify(parent, taxa, cnt, thr) == R.classify_counts(parent, want_pairs, thr)


def test_queries_resident_in_hbm_and_the_block_form(pkg, small, genome):
    import torch
    parent, node_taxon, nodes, queries, index = small
    mx = M64 // 4
    ws = sorted(set(h for h in M.window_hashes(genome[:3000], 21) if h <= mx))
    nodes2 = [ws[::2], ws[1::3], ws[::5]]
    idx2 = make_index(pkg, nodes2, parent, [5, 150, NO], max_hash=mx)
    dev_q = pkg.KmerMinHash(0, 21, False, 42, mx)
    dev_q.add_sequences([genome[:1500], genome[1000:3000]], True)      # accumulates in HBM
    host_q = sketch(pkg, ws[::4], max_hash=mx)
    want_dev = sorted(set(h for h in M.window_hashes(genome[:3000], 21) if h <= mx))
    check_counts(pkg, idx2, parent, [5, 150, NO], nodes2, [ws[::4], want_dev, ws[::4]], max_hash=mx, sketches=[host_q, dev_q, host_q])
    # the CSR in device memory
    qs = [sorted(q) for q in queries]
    flat = np.array([h for q in qs for h in q], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.uint64)
    t = torch.from_numpy(flat.view(np.int64)).cuda()
    got = index.lca_counts_block_dev(t.data_ptr(), off, hash_taxon=True)
    torch.cuda.synchronize()
    ref = index.lca_counts([sketch(pkg, q) for q in queries], hash_taxon=True)
    for a, b in zip(got, ref):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    shifted = index.lca_counts_block_dev(t.data_ptr(), off[3:], hash_taxon=True)   # offsets that do not start at 0
    for a, b in zip(shifted, ref[3:]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_the_budget_changes_no_result(pkg, small):
    parent, node_taxon, nodes, queries, index = small
    sketches = [sketch(pkg, q) for q in queries if q]
    one = index.lca_counts(sketches, hash_taxon=True)
    default = pkg.matrix.lca_budget()
    try:
        for budget, chunks in ((1, len(sketches)), (1500, None)):
            pkg.matrix.set_lca_budget(budget)
            before = count(pkg, "lca_chunk")
            again = index.lca_counts(sketches, hash_taxon=True)
            made = count(pkg, "lca_chunk") - before
            assert made == chunks if chunks else 1 < made < len(sketches), (budget, made)
            for a, b in zip(one, again):
                for x, y in zip(a, b):
                    assert np.array_equal(x, y)
    finally:
        pkg.matrix.set_lca_budget(0)
    assert pkg.matrix.lca_budget() == default


def test_downsample_meets_an_index_cut_on_the_host(pkg, small):
    parent, node_taxon, nodes, queries, index0 = small
    fine, coarse = M64 // 2, M64 // 8
    index = make_index(pkg, [[h for h in n if h <= fine] for n in nodes], parent, node_taxon, max_hash=fine)
    qs = [sketch(pkg, [h for h in queries[0] if h <= coarse], max_hash=coarse), sketch(pkg, queries[3]),
          sketch(pkg, [h for h in queries[4] if h <= fine], max_hash=fine)]
    got = index.lca_counts(qs, hash_taxon=True, downsample=True)
    for mx, k, q in ((coarse, 0, queries[0]), (fine, 1, queries[3]), (fine, 2, queries[4])):
        cut_nodes = [[h for h in n if h <= mx] for n in nodes]
        rebuilt = make_index(pkg, cut_nodes, parent, node_taxon, max_hash=mx)
        want = rebuilt.lca_counts([sketch(pkg, [h for h in q if h <= mx], max_hash=mx)], hash_taxon=True)[0]
        for x, y in zip(got[k], want):
            assert np.array_equal(x, y)
        pairs, per = R.counts(parent, node_taxon, R.owners_of(cut_nodes), [h for h in q if h <= mx])
        assert list(zip(got[k][0].tolist(), got[k][1].tolist())) == pairs and got[k][2].tolist() == per
    assert index.downsample(max_hash=coarse).has_taxonomy, "a cut index inherits the taxonomy"


def test_the_lowest_failing_query_is_reported_and_nothing_is_written(pkg, small):
    parent, node_taxon, nodes, queries, index = small
    good = sketch(pkg, queries[0])
    cases = [([good, pkg.KmerMinHash(0, 31, False, 42, M64), pkg.KmerMinHash(500, 21, False, 42, 0)], 101, "query 1"),
             ([good, good, pkg.KmerMinHash(500, 21, False, 42, 0), pkg.KmerMinHash(0, 31, False, 42, M64)], 3, "query 2"),
             ([pkg.KmerMinHash(0, 21, False, 42, M64 // 2), good], 103, "query 0")]
    L = pkg.lib()
    for qs, code, words in cases:
        arr = (C.c_void_p * len(qs))(*[q._p for q in qs])
        c_off = np.full(len(qs) + 1, 9, dtype=np.uint64)
        q_off = np.full(len(qs) + 1, 9, dtype=np.uint64)
        per = np.full(sum(len(q) for q in qs) + 1, 9, dtype=np.uint32)
        tp, cp = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)()
        with pytest.raises(pkg.SourmashError) as ei:
            pkg.errors.call(L.smh_index_lca_many, index._h, arr, len(qs), c_off.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(tp),
                            C.byref(cp), q_off.ctypes.data_as(C.POINTER(C.c_uint64)), per.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert ei.value.code == code and words in ei.value.message, ei.value.message
        assert set(c_off.tolist()) == {9} and set(q_off.tolist()) == {9} and set(per.tolist()) == {9} and not tp and not cp
    check_counts(pkg, index, parent, node_taxon, nodes, queries[:2])


# ---------------------------------------------------------------------------------- the records route

def test_hit_runs_around_the_lane_limit_and_the_wave(pkg, genome, geometry):
    lane = geometry[1]
    rng = random.Random(6)
    parent = bushy(rng, 300)
    node_taxon = [rng.randrange(300) for _ in range(29)] + [NO]
    rec = genome[1000:1400]
    ws = M.window_hashes(rec, 21)
    assert len(set(ws)) == len(ws) == 380
    nodes = [[] for _ in range(30)]
    for h in ws:
        for node in rng.sample(range(30), rng.choice([1, 1, 2, 12])):
            nodes[node].append(h)
    records = [genome[3000:3100]]                                        # 0 hits
    for runs in (1, 2, lane - 1, lane, lane + 1, 63, 64, 65, 129, 380):
        records.append(rec[:runs + 20])                                  # `runs` windows, all of them hits
    records += [genome[:20], b"", rec[:100] + b"N" + rec[101:200], rec[:50].lower()]
    index = make_index(pkg, nodes, parent, node_taxon)
    rows = check_records(pkg, index, parent, node_taxon, nodes, records)
    assert rows[0][2:] == (0, 0, NO, 0) and rows[0][0] == 80
    assert [r[1] for r in rows[1:11]] == [1, 2, lane - 1, lane, lane + 1, 63, 64, 65, 129, 380]
    assert rows[11] == rows[12] == (0, 0, 0, 0, NO, 0)
    assert {r[5] for r in rows} == {0, 1, 2}
    # a record whose hits all belong to the node without a lineage: hit, unassigned
    lone = [[] for _ in range(30)]
    lone[29] = ws[:40]
    lone[3] = ws[200:203]
    idx2 = make_index(pkg, lone, parent, node_taxon)
    rows = check_records(pkg, idx2, parent, node_taxon, lone, [rec[:60], rec, rec[200:223]])
    assert rows[0][2:] == (40, 0, NO, 0) and rows[1][2:4] == (43, 3) and rows[2][4:] == (node_taxon[3], 1)


def test_chain_fork_and_ancestor_through_records(pkg, genome):
    #  0 - 1 - 2 - 3        4 hangs off 1, 5 off 0
    parent = [0, 0, 1, 2, 1, 0]
    recs = [genome[i:i + 60] for i in range(0, 600, 100)]
    ws = [M.window_hashes(r, 21) for r in recs]
    node_taxon = [1, 2, 3, 4, 5, 0]
    nodes = [[ws[0][0], ws[2][0]],                    # taxon 1
             [ws[0][1], ws[1][0], ws[3][0]],          # taxon 2
             [ws[0][2], ws[2][1], ws[3][0]],          # taxon 3
             [ws[1][1], ws[2][2]],                    # taxon 4
             [ws[4][0]],                              # taxon 5
             [ws[5][0], ws[4][1]]]                    # the root
    index = make_index(pkg, nodes, parent, node_taxon)
    rows = check_records(pkg, index, parent, node_taxon, nodes, recs)
    assert rows[0][4:] == (3, 1), "a chain gives the deepest taxon, found"
    assert rows[1][4:] == (1, 2), "a fork gives the branching point, disagree"
    assert rows[2][4:] == (1, 2), "an ancestor plus a fork below it"
    assert rows[3][4:] == (2, 1), "a hash held by taxa 2 and 3 has their lca"
    assert rows[4][4:] == (5, 1) and rows[5][4:] == (0, 1), "root only"


def test_more_records_than_one_grid_dimension(pkg, pyoracle):
    pool = [pyoracle.synth_dna(40 * i, 25, 77) for i in range(300)]
    rng = random.Random(5)
    records = [pool[rng.randrange(300)] for _ in range(70000)]
    records[0], records[65535], records[65536], records[69999] = pool[0], pool[1], pool[2], pool[3]
    hs = [M.window_hashes(p, 21) for p in pool]
    nodes = [[h for w in hs[0:300:2] for h in w[:2]], [h for w in hs[1:300:3] for h in w], [hs[3][4]], []]
    parent, node_taxon = [0, 0, 1, 1, 0], [2, 3, 4, NO]
    index = make_index(pkg, nodes, parent, node_taxon)
    owners = R.owners_of(nodes)
    per_pool = {p: R.classify_record(parent, node_taxon, owners, p, 21, 42, M64) for p in set(records)}
    got = rows_of(index.lca_classify_records(records))
    assert got == [per_pool[r] for r in records]
    assert got[69999][3] >= 1 and {0, 1} <= {g[5] for g in got}


@pytest.mark.parametrize("ksize", [21, 31, 33])
def test_ksizes(pkg, genome, ksize):
    rng = random.Random(ksize)
    records = [genome[i:i + 150] for i in range(0, 3000, 97)] + [genome[:ksize - 1], genome[:ksize], b""]
    ws = M.window_hashes(genome[:3200], ksize)
    nodes = [ws[0:1000:3], ws[500:2500:5], ws[2000::2], []]
    parent = bushy(rng, 20)
    node_taxon = [3, 11, 17, 5]
    index = make_index(pkg, nodes, parent, node_taxon, ksize=ksize)
    check_records(pkg, index, parent, node_taxon, nodes, records, ksize=ksize)


def test_routes_agree_and_the_pair_budget_changes_nothing(pkg, genome):
    import torch
    rng = random.Random(9)
    records = [genome[i:i + 90 + i % 7] for i in range(0, 3000, 75)] + [genome[:10]]
    ws = M.window_hashes(genome[:3200], 21)
    nodes = [ws[::3], ws[1::4], ws[100:400]]
    parent, node_taxon = bushy(rng, 12), [4, 9, 11]
    index = make_index(pkg, nodes, parent, node_taxon)
    host = index.lca_classify_records(records)
    flat = b"".join(records)
    off = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.uint64)
    t = torch.from_numpy(np.frombuffer(flat, dtype=np.uint8).copy()).cuda()
    dev = index.lca_classify_records((t.data_ptr(), len(flat), off))
    torch.cuda.synchronize()
    text = b"".join(b">r%d some words\n" % i + r[:40] + b"\n" + (r[40:] + b"\n" if r[40:] else b"") for i, r in enumerate(records))
    rec = index.lca_classify_records(pkg.fastx.Records.parse(text))
    for f in FIELDS:
        assert np.array_equal(getattr(host, f), getattr(dev, f)), f
        assert np.array_equal(getattr(host, f), getattr(rec, f)), f
    assert rows_of(host) == R.classify_records(parent, node_taxon, nodes, records, 21, 42, M64)
    try:
        for budget in (150, 1):
            pkg.matrix.set_match_pair_budget(budget)
            folds = count(pkg, "match_fold")
            again = index.lca_classify_records(records)
            assert count(pkg, "match_fold") - folds >= len(records) - 1
            for f in FIELDS:
                assert np.array_equal(getattr(host, f), getattr(again, f)), (budget, f)
    finally:
        pkg.matrix.set_match_pair_budget(0)
    # a cut index is an index like any other, and carries the taxonomy
    coarse = make_index(pkg, nodes, parent, node_taxon, max_hash=M64 // 2).downsample(max_hash=M64 // 8)
    assert coarse.has_taxonomy
    want = R.classify_records(parent, node_taxon, [[h for h in n if h <= M64 // 8] for n in nodes], records, 21, 42, M64 // 8)
    assert rows_of(coarse.lca_classify_records(records)) == want


def test_second_witness_match_hits_and_the_literal_rule(pkg, pyoracle):
    mx = M64 // 2
    ref = pyoracle.synth_dna(0, 12000, 33)
    rng = random.Random(8)
    records = [ref[s:s + 150] for s in (rng.randrange(0, 11850) for _ in range(196))] + [b"", ref[:20], ref[:21], b"ACGTN" * 30]
    parent = bushy(rng, 120)
    sketches, node_taxon = [], []
    for i in range(50):
        part = pkg.KmerMinHash(0, 21, False, 42, mx)
        # consecutive pieces, every fifth one also a stretch somewhere else: a read inside a piece is found, one across two
        # pieces whose taxa lie on different branches disagrees
        part.add_sequence(ref[240 * i:240 * i + 240], True)
        if i % 5 == 0:
            a = rng.randrange(0, 11000)
            part.add_sequence(ref[a:a + 1000], True)
        sketches.append(part)
        node_taxon.append(rng.randrange(120) if i % 9 else NO)
    index = pkg.index.ResidentIndex(sketches)
    index.set_taxonomy(parent, node_taxon)
    owners = R.owners_of([m.mins for m in sketches])
    res = index.lca_classify_records(records)
    m = index.match(records, hits=True)
    for r in range(len(records)):
        hits = m.hit_hashes[int(m.hit_offsets[r]):int(m.hit_offsets[r + 1])].tolist()
        taxa = [t for t in (R.hash_taxon(parent, node_taxon, owners, h) for h in hits) if t != NO]
        assert (int(res.taxon[r]), int(res.status[r])) == R.find_lca(parent, taxa), r
        assert int(res.assigned_distinct[r]) == len(taxa) and int(res.hit_distinct[r]) == len(hits)
    assert len(set(res.status.tolist())) == 3 and len(set(res.taxon.tolist())) > 10


# ---------------------------------------------------------------------------------- lifecycle

def test_table_lifecycle_timers_and_refusals(pkg, genome):
    L = pkg.lib()
    ws = M.window_hashes(genome[:500], 21)
    nodes = [ws[::2], ws[1::2], ws[::5]]
    parent, node_taxon = [0, 0, 1, 1], [2, 3, NO]
    records = [genome[:200], genome[200:500]]
    index = pkg.index.ResidentIndex([sketch(pkg, n) for n in nodes])
    assert not index.has_taxonomy
    for call in (lambda: index.lca_counts([sketch(pkg, ws[:9])]), lambda: index.lca_classify_records(records)):
        with pytest.raises(pkg.SourmashError) as ei:
            call()
        assert ei.value.code == 3 and "taxonomy" in ei.value.message
    for bad_parent, bad_taxon, words in (([0, 0, 2], node_taxon, "parent[2] is 2"), (parent, [2, 3], "n_nodes is 2"),
                                         (parent, [2, 4, NO], "node_taxon[1] is 4"), ([1, 0], node_taxon, "parent[0] is 1")):
        with pytest.raises(pkg.SourmashError) as ei:
            index.set_taxonomy(bad_parent, bad_taxon)
        assert ei.value.code == 3 and words in ei.value.message
        assert not index.has_taxonomy
    index.set_taxonomy(parent, node_taxon)
    assert index.has_taxonomy
    L.smh_profile_enable(1)
    try:
        L.smh_profile_reset()
        built, dirs = count(pkg, "lca_table_built"), count(pkg, "match_directory_built")
        for _ in range(3):
            check_counts(pkg, index, parent, node_taxon, nodes, [ws[:50], ws[100:]])
            check_records(pkg, index, parent, node_taxon, nodes, records)
        assert count(pkg, "lca_table_built") == built + 1, "the table is built once over many calls"
        assert count(pkg, "match_directory_built") == dirs + 1
        for name in ("lca_table", "lca_probe", "lca_records"):
            ms = C.c_double()
            L.smh_profile_get(name.encode(), C.byref(ms), None)
            assert ms.value > 0 and count(pkg, name) >= 1, name
    finally:
        L.smh_profile_enable(0)
    flipped = [3, 2, 2]
    index.set_taxonomy(parent, flipped)
    check_records(pkg, index, parent, flipped, nodes, records)
    check_counts(pkg, index, parent, flipped, nodes, [ws[:50]])
    assert count(pkg, "lca_table_built") == built + 2, "rebuilt after set_taxonomy"
    assert L.smh_release_workspace() == 0
    check_counts(pkg, index, parent, flipped, nodes, [ws[:50]])
    assert count(pkg, "lca_table_built") == built + 3, "rebuilt after smh_release_workspace"
    # the index's own refusals: as match refuses, and the sketch route's
    protein = pkg.index.ResidentIndex([pkg.KmerMinHash(0, 21, True, 42, 1 << 62)])
    protein.set_taxonomy([0], [0])
    with pytest.raises(pkg.SourmashError) as ei:
        protein.lca_classify_records(records)
    assert ei.value.code == 3 and ei.value.message.startswith("match: ")
    mixed = pkg.index.ResidentIndex([sketch(pkg, ws[:5]), sketch(pkg, ws[:5], max_hash=M64 // 2)])
    mixed.set_taxonomy([0], [0, 0])
    with pytest.raises(pkg.SourmashError) as ei:
        mixed.lca_counts([sketch(pkg, ws[:9])])
    assert ei.value.code == 3 and "same ksize" in ei.value.message
    check_records(pkg, index, parent, flipped, nodes, records)
