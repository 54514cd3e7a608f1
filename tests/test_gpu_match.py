"""Matching records against a resident index on the device against tests/match_restatement.py: every row,
and the hit list where asked, must be EQUAL.  The shapes stand on both sides of the sizes smh_match_geometry reports (the
probe's LDS sample, the LDS pair capacity of the tally) and of the limits around them (one grid dimension of records, one
record much longer than a tile, the pair budget).  A second witness that shares nothing with the restatement -- a sketch per
record and the N x M compare -- is at the end."""
import ctypes as C
import random

import numpy as np
import pytest

import match_restatement as R

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
FIELDS = ("windows", "distinct", "hit_windows", "hit_distinct", "best", "best_common")


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


def make_index(pkg, nodes, ksize=21, max_hash=M64, seed=42):
    sketches = []
    for hashes in nodes:
        mh = pkg.KmerMinHash(0, ksize, False, seed, max_hash)
        if len(hashes):
            mh.add_many(np.array(sorted(hashes), dtype=np.uint64))
        sketches.append(mh)
    return pkg.index.ResidentIndex(sketches)


def rows_of(res):
    return list(zip(*[[int(x) for x in getattr(res, f)] for f in FIELDS]))


def check(pkg, records, nodes, ksize=21, max_hash=M64, seed=42, index=None, owners=None):
    """the library's answer (with the hit list) next to the restatement's; returns the rows"""
    index = index or make_index(pkg, nodes, ksize, max_hash, seed)
    kept = owners if owners is not None else R.owners_of([[h for h in node if h <= max_hash] for node in nodes])
    want_rows, want_off, want_flat = R.match(records, ksize, seed, max_hash, kept)
    res = index.match(records, hits=True)
    got = rows_of(res)
    assert len(got) == len(want_rows)
    bad = [i for i in range(len(got)) if got[i] != want_rows[i]]
    assert not bad, (bad[:5], [got[i] for i in bad[:5]], [want_rows[i] for i in bad[:5]])
    assert res.hit_offsets.tolist() == want_off
    assert res.hit_hashes.tolist() == want_flat
    plain = index.match(records)
    assert plain.hit_offsets is None and plain.hit_hashes is None and rows_of(plain) == got
    return got


@pytest.fixture(scope="module")
def geometry(pkg):
    lds_pairs, threads, samples = pkg.matrix.match_geometry()
    assert lds_pairs >= 64 and threads % 64 == 0 and samples >= 64
    return lds_pairs, threads, samples


@pytest.fixture(scope="module")
def genome(pyoracle):
    return pyoracle.synth_dna(0, 6000, 21)


def unrelated(rng, n):
    """n distinct hashes that no window of the tests has (the top bit pattern is fixed; window hashes that collide are none in practice)"""
    out = set()
    while len(out) < n:
        out.add(rng.getrandbits(64) | 1)
    return sorted(out)


# ---------------------------------------------------------------------------------- records

def test_short_records_and_the_record_boundary(pkg, genome):
    a, b = genome[:60], genome[60:130]
    straddle = R.kmer_hash(a[-10:] + b[:11])
    inside = R.window_hashes(a, 21)
    assert straddle not in inside and straddle not in R.window_hashes(b, 21)
    nodes = [[straddle, inside[3]], [inside[3], inside[39]], [5, 7]]
    records = [b"", genome[:20], genome[:21], genome[:22], a, b, b"", a + b, b"A"]
    rows = check(pkg, records, nodes)
    assert rows[0] == rows[1] == (0, 0, 0, 0, R.MISS, 0)
    assert rows[2][0] == 1 and rows[3][0] == 2
    assert rows[4][3] == 2 and rows[5][3] == 0, "the planted k-mer across the boundary counted"
    assert rows[7][3] == 3 and rows[7][4:] == (0, 2)


def test_repeats_lowercase_and_n(pkg, genome):
    k = genome[200:221]
    h = R.kmer_hash(k)
    three = k + genome[300:310] + k + genome[400:407] + k
    rec = genome[500:600]
    n_first, n_last = b"N" + rec[1:], rec[:-1] + b"N"
    nodes = [[h] + R.window_hashes(rec, 21)[::3], R.window_hashes(rec, 21)[:2] + R.window_hashes(rec, 21)[-2:]]
    rows = check(pkg, [three, three.lower(), rec, rec.lower(), n_first, n_last, b"ACGTN" * 30, rec[:50] + b"n" + rec[51:]], nodes)
    assert rows[0][2] == 3 and rows[0][3] == 1 and rows[0] == rows[1] and rows[2] == rows[3]
    assert rows[4][0] == rows[5][0] == 79 and rows[6] == (0, 0, 0, 0, R.MISS, 0) and rows[7][0] == 80 - 21


def test_more_records_than_one_grid_dimension(pkg, pyoracle):
    pool = [pyoracle.synth_dna(40 * i, 25, 77) for i in range(300)]
    rng = random.Random(5)
    records = [pool[rng.randrange(300)] for _ in range(70000)]
    records[0], records[65535], records[65536], records[69999] = pool[0], pool[1], pool[2], pool[3]
    hs = [R.window_hashes(p, 21) for p in pool]
    nodes = [[h for w in hs[0:300:2] for h in w[:2]], [h for w in hs[1:300:3] for h in w], [hs[3][4]], []]
    rows = check(pkg, records, nodes)
    assert rows[69999][3] >= 1 and len(rows) == 70000


def test_one_long_record(pkg, pyoracle):
    block = pyoracle.synth_dna(1000, 30000, 9)
    rec = block * 10
    assert len(rec) == 300000
    hs = R.window_hashes(block, 21)
    nodes = [hs[::7], hs[5::11] + unrelated(random.Random(1), 500), hs[:100]]
    rows = check(pkg, [block[:500], rec, block[29000:]], nodes)
    assert rows[1][0] == 300000 - 20 and rows[1][1] < rows[1][0]


@pytest.mark.parametrize("ksize", [21, 31, 33])
def test_ksizes(pkg, genome, ksize):
    records = [genome[i:i + 150] for i in range(0, 3000, 97)] + [genome[:ksize - 1], genome[:ksize], b""]
    ws = R.window_hashes(genome[:3200], ksize)
    nodes = [ws[0:1000:3], ws[500:2500:5], ws[2000::2], []]
    check(pkg, records, nodes, ksize=ksize)


# ---------------------------------------------------------------------------------- sampling

def test_sampling_bounds(pkg, genome):
    records = [genome[i:i + 200] for i in range(0, 4000, 150)]
    ws = sorted(set(R.window_hashes(genome[:4300], 21)))
    nodes = [ws[::2], ws[::3], ws[1::5]]
    rows = check(pkg, records, nodes, max_hash=(1 << 64) // 4)
    assert 0 < sum(r[0] for r in rows) < sum(len(r) - 20 for r in records)
    mid = ws[len(ws) // 2]            # one window's own hash: that window is sampled
    at = check(pkg, records, nodes, max_hash=mid)
    below = check(pkg, records, nodes, max_hash=mid - 1)
    assert sum(r[0] for r in at) > sum(r[0] for r in below)
    none = check(pkg, records, nodes, max_hash=ws[0] - 1)
    assert all(r == (0, 0, 0, 0, R.MISS, 0) for r in none)
    only = check(pkg, records, nodes, max_hash=ws[0])
    assert sum(r[1] for r in only) >= 1 and all(r[1] <= 1 for r in only)


# ---------------------------------------------------------------------------------- the directory probe

def test_probe_at_the_ends_of_the_directory(pkg, genome):
    rec = genome[1000:1200]
    ws = sorted(set(R.window_hashes(rec, 21)))
    rows = check(pkg, [rec], [ws[1:-1:2], ws[2:-1:2]])       # ws[0] below U[0], ws[1] == U[0], ws[-2] == U[last], ws[-1] above
    assert rows[0][3] == len(ws) - 2
    check(pkg, [rec, genome[:100]], [[ws[40]]])              # a directory of one hash
    check(pkg, [rec], [[ws[0]], [ws[-1]]])
    check(pkg, [rec], [[1], [M64]])                          # everything lies strictly inside, nothing hits


@pytest.mark.parametrize("delta", [-1, 0, 1, "x4"])
def test_directory_around_the_lds_sample(pkg, genome, geometry, delta):
    samples = geometry[2]
    size = 4 * samples + 3 if delta == "x4" else samples + delta
    records = [genome[i:i + 120] for i in range(0, 2400, 100)]
    ws = sorted(set(R.window_hashes(genome[:2600], 21)))
    planted = ws[::4]
    assert len(planted) < size
    rest = unrelated(random.Random(size), size - len(planted))
    assert not set(rest) & set(ws)
    everything = sorted(planted + rest)
    assert len(set(everything)) == size
    nodes = [everything[0::3], everything[1::3], everything[2::3] + everything[:50], everything[::97]]
    check(pkg, records, nodes)


def test_empty_and_identical_nodes(pkg, genome):
    records = [genome[i:i + 100] for i in range(0, 1000, 100)]
    ws = R.window_hashes(genome[:1100], 21)
    rows = check(pkg, records, [[], [], []])
    assert all(r[2:] == (0, 0, R.MISS, 0) and r[0] == 80 for r in rows)
    check(pkg, records, [[], ws[::5], [], ws[1::5], []])
    rows = check(pkg, records, [ws[::4]] * 6 + [[]])
    assert all(r[4] == 0 for r in rows)                      # equal owner lists: the tie goes to node 0
    rows = check(pkg, records, [ws[::2]])                    # an index of one node
    assert all(r[4] == 0 and r[5] == r[3] for r in rows)
    none = make_index(pkg, [ws[::2]]).match([], hits=True)   # a batch without records
    assert rows_of(none) == [] and none.hit_offsets.tolist() == [0] and none.hit_hashes.size == 0


# ---------------------------------------------------------------------------------- the tally

def pairs_of(record, nodes, ksize=21):
    own = R.owners_of(nodes)
    return sum(len(own[h]) for h in set(R.window_hashes(record, ksize)) if h in own)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_owner_pairs_around_the_lds_capacity(pkg, genome, geometry, delta):
    cap = geometry[0]
    n_nodes = 40
    rec = genome[2000:2000 + cap // n_nodes + 21 + 150]
    ws = R.window_hashes(rec, 21)
    assert len(set(ws)) == len(ws)
    full = cap // n_nodes - 1                                # hashes held by every node
    single = cap + delta - full * n_nodes                    # hashes held by node 7 alone
    assert 0 < single <= len(ws) - full
    nodes = [list(ws[:full]) for _ in range(n_nodes)]
    nodes[7] = nodes[7] + ws[full:full + single]
    assert pairs_of(rec, nodes) == cap + delta
    rows = check(pkg, [genome[:100], rec, rec[:60], rec], nodes)
    assert rows[1] == rows[3] and rows[1][4:] == (7, full + single)


@pytest.fixture(scope="module")
def wide(pkg, genome):
    """3 000 nodes: one hash held by all of them, ties between node 5 and node 2 000, the last node best"""
    recs = [genome[i:i + 100] for i in range(0, 1200, 100)]
    ws = [R.window_hashes(r, 21) for r in recs]
    everyone = [ws[0][0], ws[1][0], ws[2][0], ws[3][0]] + [w[1] for w in ws[4:]]
    nodes = [list(everyone) for _ in range(3000)]
    for node in (5, 2000):
        nodes[node] = nodes[node] + [ws[1][5], ws[1][6], ws[6][7]]          # record 1 (dense) and record 6 (dense): a tie
    nodes[2999] = nodes[2999] + [ws[2][9], ws[2][10], ws[7][3]]             # the last node best
    tie_lds = genome[3000:3100]                                            # no hash of `everyone`: the LDS regime
    t = R.window_hashes(tie_lds, 21)
    for node in (5, 2000):
        nodes[node] = nodes[node] + [t[2], t[3]]
    last_lds = genome[3200:3300]
    nodes[2999] = nodes[2999] + R.window_hashes(last_lds, 21)[:4]
    records = recs + [tie_lds, last_lds, genome[4000:4100]]
    return records, nodes, make_index(pkg, nodes), R.owners_of(nodes)


def test_a_hash_held_by_every_node_ties_and_the_last_node(pkg, wide, geometry):
    records, nodes, index, owners = wide
    assert pairs_of(records[0], nodes) >= 3000 > geometry[0]
    before = count(pkg, "match_dense_round")
    rows = check(pkg, records, nodes, index=index, owners=owners)
    assert count(pkg, "match_dense_round") > before
    assert rows[0][4:] == (0, 1)                  # 3 000 nodes tie at one hash: node 0
    assert rows[1][4:] == (5, 3) and rows[6][4:] == (5, 2)      # dense regime: 5 and 2 000 tie
    assert rows[2][4:] == (2999, 3) and rows[7][4:] == (2999, 2)
    assert rows[12][4:] == (5, 2) and rows[13][4:] == (2999, 4)   # LDS regime
    assert rows[14] == (80, 80, 0, 0, R.MISS, 0)


def test_the_pair_budget_changes_no_result(pkg, wide):
    records, nodes, index, owners = wide
    one_round = index.match(records, hits=True)
    default = pkg.matrix.match_pair_budget()
    try:
        for budget in (7000, 150, 1):
            pkg.matrix.set_match_pair_budget(budget)
            folds, rounds = count(pkg, "match_fold"), count(pkg, "match_dense_round")
            again = index.match(records, hits=True)
            assert count(pkg, "match_dense_round") - rounds >= 6, "the dense records fitted one round"
            assert count(pkg, "match_fold") - folds >= (1 if budget == 7000 else len(records))   # 101 per record of 100 bases
            for f in FIELDS + ("hit_offsets", "hit_hashes"):
                assert np.array_equal(getattr(again, f), getattr(one_round, f)), (budget, f)
    finally:
        pkg.matrix.set_match_pair_budget(0)
    assert pkg.matrix.match_pair_budget() == default
    check(pkg, records, nodes, index=index, owners=owners)


# ---------------------------------------------------------------------------------- a second witness, routes, refusals

def test_second_witness_sketch_per_record_and_the_matrix(pkg, pyoracle):
    mx = M64 // 2
    ref = pyoracle.synth_dna(0, 12000, 33)
    rng = random.Random(8)
    records = [ref[s:s + 150] for s in (rng.randrange(0, 11850) for _ in range(196))] + [b"", ref[:20], ref[:21], b"ACGTN" * 30]
    assert len(records) == 200
    nodes = []
    for i in range(50):
        part = pkg.KmerMinHash(0, 21, False, 42, mx)
        a = rng.randrange(0, 11000)
        part.add_sequence(ref[a:a + rng.choice([10, 300, 1000, 4000])], True)
        part.add_many(np.array(unrelated(rng, 40), dtype=np.uint64))
        nodes.append(part)
    index = pkg.index.ResidentIndex(nodes)
    res = index.match(records, hits=True)
    per_record = [pkg.KmerMinHash(0, 21, False, 42, mx) for _ in records]
    pkg.KmerMinHash.add_sequences_grouped(per_record, records, list(range(200)), True)
    cc = pkg.index.ResidentIndex(per_record).compare(index, want=("count_common",))["count_common"]
    union = np.unique(np.concatenate([m.mins_np() for m in nodes]))
    for r in range(200):
        mine = per_record[r].mins_np()
        assert int(res.distinct[r]) == mine.size
        assert int(res.hit_distinct[r]) == np.intersect1d(mine, union).size
        assert int(res.best_common[r]) == int(cc[r].max())
        assert int(res.best[r]) == (int(cc[r].argmax()) if cc[r].max() else R.MISS)
        assert res.hit_hashes[int(res.hit_offsets[r]):int(res.hit_offsets[r + 1])].tolist() == np.intersect1d(mine, union).tolist()
    assert int(res.hit_distinct.sum()) > 100 and len(set(res.best.tolist())) > 5


def test_routes_agree(pkg, genome):
    import torch
    records = [genome[i:i + 90 + i % 7] for i in range(0, 3000, 75)] + [genome[:10]]
    ws = R.window_hashes(genome[:3200], 21)
    nodes = [ws[::3], ws[1::4], ws[100:400]]
    index = make_index(pkg, nodes)
    host = index.match(records, hits=True)
    flat = b"".join(records)
    off = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.uint64)
    t = torch.from_numpy(np.frombuffer(flat, dtype=np.uint8).copy()).cuda()
    dev = index.match((t.data_ptr(), len(flat), off), hits=True)
    torch.cuda.synchronize()
    text = b"".join(b">r%d some words\n" % i + r[:40] + b"\n" + (r[40:] + b"\n" if r[40:] else b"") for i, r in enumerate(records))
    parsed = pkg.fastx.Records.parse(text)
    assert len(parsed) == len(records)
    rec = index.match(parsed, hits=True)
    for f in FIELDS + ("hit_offsets", "hit_hashes"):
        assert np.array_equal(getattr(host, f), getattr(dev, f)), f
        assert np.array_equal(getattr(host, f), getattr(rec, f)), f
    assert rows_of(host) == R.match(records, 21, 42, M64, nodes)[0]
    # a cut index is an index like any other
    coarse = make_index(pkg, nodes, max_hash=M64 // 2).downsample(max_hash=M64 // 8)
    got = rows_of(coarse.match(records))
    assert got == R.match(records, 21, 42, M64 // 8, [[h for h in n if h <= M64 // 8] for n in nodes])[0]


def test_refusals_leave_the_library_usable(pkg, genome):
    mx = 1 << 62
    dna = lambda: pkg.KmerMinHash(0, 21, False, 42, mx)
    records = [genome[:100], genome[100:250]]
    cases = {"protein": [pkg.KmerMinHash(0, 21, True, 42, mx), pkg.KmerMinHash(0, 21, True, 42, mx)],
             "num": [dna(), pkg.KmerMinHash(500, 21, False, 42, 0)],
             "two max_hash": [dna(), pkg.KmerMinHash(0, 21, False, 42, mx // 2)],
             "ksize": [dna(), pkg.KmerMinHash(0, 31, False, 42, mx)],
             "no node": []}
    for what, sketches in cases.items():
        with pytest.raises(pkg.SourmashError) as ei:
            pkg.index.ResidentIndex(sketches).match(records, hits=True)
        assert ei.value.code == 3 and ei.value.message.startswith("match: "), what
        ws = R.window_hashes(genome[:250], 21)
        check(pkg, records, [ws[::2], ws[::3]], max_hash=mx)


def test_the_kernels_ran(pkg, genome):
    L = pkg.lib()
    ws = R.window_hashes(genome[:500], 21)
    index = make_index(pkg, [ws[::2], ws[1::2]])
    L.smh_profile_enable(1)
    try:
        L.smh_profile_reset()
        built = count(pkg, "match_directory_built")
        index.match([genome[:200], genome[200:500]])
        index.match([genome[:200]])
        assert count(pkg, "match_probe") == 2 and count(pkg, "match_tally") == 2
        assert count(pkg, "match_directory_built") == built + 1, "the directory is built once per index"
    finally:
        L.smh_profile_enable(0)
