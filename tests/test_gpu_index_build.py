"""Building a resident index from records on the device (smh_index_from_*; ResidentIndex.from_records) and concatenating
resident indexes (smh_index_concat; ResidentIndex.concat).  Two witnesses: the plain-Python restatement
(index_build_restatement.py) and the route that existed before -- add_sequences_grouped(force=True) into fresh sketches, then
ResidentIndex(sketches).read().  Everything is an integer, so offsets, hashes and abundances must be EQUAL.  max_hash is
2^64 - 1 unless a test says otherwise: every window is sampled and the candidate counts are exact; the sizes stand on both
sides of the tile smh_index_build_geometry reports.

Not run at its size: the refusal of a (group, hash) count of 2^32 or more (4 Gi windows of one k-mer) and the refusal of more
than 2^31 - 1 (group, hash) pairs (16 GiB of hashes); their conditions are in test_index_build_rules.py."""
import ctypes as C

import numpy as np
import pytest

import index_build_restatement as IB

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
MOLECULES = {"DNA": None, "protein": "protein", "dayhoff": "dayhoff", "hp": "hp"}


def like_of(pkg, ksize=21, molecule="DNA", track=True, max_hash=M64, seed=42):
    return pkg.KmerMinHash(0, ksize, False, seed, max_hash, track, alphabet=MOLECULES[molecule])


def params(like):
    return dict(num=0, ksize=like.ksize, molecule=like.molecule, seed=like.seed, max_hash=like.max_hash, track=bool(like.track_abundance))


def dna(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))


def amino(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8), size=n))


def triple(index):
    off, h, ab = index.read()
    return off.tolist(), h.tolist(), None if ab is None else ab.tolist()


def host_route(pkg, like, records, groups, G, amino_input=False):
    """the route that existed before: fresh sketches filled through the grouped fold, uploaded as an index"""
    p = params(like)
    sk = [like_of(pkg, p["ksize"], p["molecule"], p["track"], p["max_hash"], p["seed"]) for _ in range(G)]
    groups = list(range(len(records))) if groups is None else list(groups)
    if amino_input:
        for g in range(G):
            mine = [r for r, gg in zip(records, groups) if gg == g]
            if mine:
                sk[g].add_proteins(mine)
    elif records:
        pkg.KmerMinHash.add_sequences_grouped(sk, records, groups, True)
    return pkg.index.ResidentIndex(sk)


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


@pytest.fixture(scope="module")
def T(pkg):
    tile, threads = C.c_uint32(), C.c_uint32()
    pkg.lib().smh_index_build_geometry(C.byref(tile), C.byref(threads))
    assert tile.value % threads.value == 0 and 64 <= threads.value <= tile.value <= 1 << 16
    return tile.value


@pytest.fixture
def budget(pkg):
    L = pkg.lib()
    yield L.smh_index_build_set_budget
    L.smh_index_build_set_budget(0)


def build_and_check(pkg, like, records, groups, G, amino_input=False, restate=True, host=True):
    built = pkg.index.ResidentIndex.from_records(records, like, groups, G, amino=amino_input)
    got = triple(built)
    if restate:
        assert got == IB.build(records, None if groups is None else list(groups), G, params(like), IB.AMINO if amino_input else IB.NUCLEOTIDE)
    if host:
        assert got == triple(host_route(pkg, like, records, groups, G, amino_input))
    assert len(built) == G and built.has_abundances == bool(like.track_abundance)
    assert built.sizes().tolist() == np.diff(np.array(got[0], dtype=np.int64)).tolist()
    return built


@pytest.mark.parametrize("track", [True, False])
@pytest.mark.parametrize("ksize,molecule,amino_input", [
    (21, "DNA", False), (31, "DNA", False), (41, "DNA", False),            # the rolling kernel twice, the byte-wise one
    (30, "protein", False), (27, "dayhoff", False),                        # translated
    (30, "protein", True), (27, "hp", True)])                              # amino input
def test_parity_grid_groups_given(pkg, ksize, molecule, amino_input, track):
    rng = np.random.default_rng(ksize * 7 + track)
    gen = amino if amino_input else dna
    lens = [0, 5, 400, 90, 700, 33, 260, ksize, ksize - 1, 150]
    records = [gen(rng, n) for n in lens]
    records[4] = records[2][:300] + records[4][300:]          # a stretch shared by two groups and repeated inside one
    records[6] = records[2][:200] + records[6][200:]
    if not amino_input:
        records[3] = records[3][:40] + b"N" + records[3][41:]
    groups = [3, 0, 1, 4, 2, 1, 1, 0, 4, 3]
    build_and_check(pkg, like_of(pkg, ksize, molecule, track), records, groups, 6, amino_input)


@pytest.mark.parametrize("ksize,molecule,amino_input", [(21, "DNA", False), (27, "dayhoff", False), (30, "protein", True)])
def test_parity_one_node_per_record_without_group_ids(pkg, ksize, molecule, amino_input):
    rng = np.random.default_rng(5)
    gen = amino if amino_input else dna
    records = [gen(rng, n) for n in (120, 0, 64, 10, 333)]
    build_and_check(pkg, like_of(pkg, ksize, molecule), records, None, 5, amino_input)
    build_and_check(pkg, like_of(pkg, ksize, molecule), records[:1], None, 1, amino_input)   # a batch of one record


def test_scaled_sampling_matches_the_grouped_route(pkg):
    rng = np.random.default_rng(9)
    records = [dna(rng, 30000) for _ in range(4)]
    build_and_check(pkg, like_of(pkg, 31, max_hash=M64 // 50), records, [0, 1, 1, 2], 3, restate=False)


def test_candidate_counts_around_the_tile(pkg, T):
    rng = np.random.default_rng(11)
    like = like_of(pkg, 21)
    long_one = dna(rng, 2 * T + 1 + 20)
    for n in (0, 1, T - 1, T, T + 1, 2 * T + 1):
        rec = long_one[:n + 20] if n else long_one[:20]
        built = build_and_check(pkg, like, [rec], [0], 1, restate=n <= T + 1)
        off, h, ab = built.read()
        assert len(h) == n and (n == 0 or ab.tolist() == [1] * n)      # distinct k-mers: every element is a head


def test_a_run_over_a_whole_tile(pkg, T):
    like = like_of(pkg, 21)
    built = pkg.index.ResidentIndex.from_records([b"A" * (2 * T + 21)], like)
    off, h, ab = built.read()
    assert off.tolist() == [0, 1] and ab.tolist() == [2 * T + 21 - 21 + 1]
    assert h.tolist() == IB.build([b"A" * 21], None, 1, params(like))[1]


def test_group_boundary_on_a_tile_edge_with_a_shared_hash(pkg, T):
    # group 0 holds exactly T candidates, so group 1 starts on the tile's edge; group 1 is the one window with group 0's largest
    # hash, so the same hash lies on both sides of the edge and only the group tells the two elements apart
    rng = np.random.default_rng(13)
    like = like_of(pkg, 21)
    first = dna(rng, T + 20)
    hs = IB.build([first], None, 1, params(like))[1]
    assert len(hs) == T
    import match_restatement as MR
    wh = MR.window_hashes(first, 21)
    p = wh.index(hs[-1])
    shared = first[p:p + 21]                                            # the window with group 0's largest hash
    records = [first, shared]
    built = build_and_check(pkg, like, records, [0, 1], 2)
    off, h, ab = built.read()
    assert off.tolist() == [0, T, T + 1] and h[T - 1] == h[T]
    # and with more behind the shared hash in group 1
    tail = dna(rng, 300)
    build_and_check(pkg, like, [first, shared, tail], [0, 1, 1], 2)


def test_three_nonempty_groups_among_seventy_thousand(pkg):
    rng = np.random.default_rng(17)
    G = 70000
    like = like_of(pkg, 21)
    records = [dna(rng, 100), dna(rng, 60), dna(rng, 80)]
    built = build_and_check(pkg, like, records, [0, 1, G - 1], G, host=False)
    sizes = built.sizes()
    assert sizes[0] == 80 and sizes[1] == 40 and sizes[G - 1] == 60 and int(sizes.sum()) == 180


def test_budget_independence(pkg, budget):
    rng = np.random.default_rng(19)
    like = like_of(pkg, 21)
    rep = dna(rng, 60)
    big = dna(rng, 200) + rep + dna(rng, 150) + rep + dna(rng, 50)      # one record over several folds, a k-mer run twice, folds apart
    records = [big, dna(rng, 100) + rep, dna(rng, 50)]
    groups = [0, 1, 0]
    want = IB.build(records, groups, 2, params(like))
    folds = {}
    for b in (1, 150, 7000, 0):
        budget(b)
        before = count(pkg, "index_build_fold")
        assert triple(pkg.index.ResidentIndex.from_records(records, like, groups, 2)) == want, "budget %d" % b
        folds[b] = count(pkg, "index_build_fold") - before
    assert folds[1] > folds[150] > 2 and folds[7000] == 1 and folds[0] == 1
    assert max(want[2]) >= 2


def test_budget_independence_of_the_translated_and_amino_arms(pkg, budget):
    rng = np.random.default_rng(23)
    recs = [dna(rng, 300), dna(rng, 200), dna(rng, 250)]
    prot = [amino(rng, 200), amino(rng, 150)]
    for like, records, groups, G, am in ((like_of(pkg, 27, "dayhoff"), recs, [1, 0, 1], 2, False), (like_of(pkg, 30, "protein"), prot, None, 2, True)):
        want = IB.build(records, groups, G, params(like), IB.AMINO if am else IB.NUCLEOTIDE)
        for b in (150, 0):
            budget(b)
            assert triple(pkg.index.ResidentIndex.from_records(records, like, groups, G, amino=am)) == want


@pytest.fixture(scope="module")
def fifty(pkg):
    """about 50 nodes that share stretches, built here and through the host"""
    rng = np.random.default_rng(29)
    like = like_of(pkg, 21, max_hash=M64 // 4)
    base = [dna(rng, 1500) for _ in range(8)]
    records, groups = [], []
    for g in range(50):
        a, b = base[g % 8], base[(g * 3 + 1) % 8]
        records += [a[(g * 13) % 400:][:900], b[:600], dna(rng, 200)]
        groups += [g, g, g]
    built = pkg.index.ResidentIndex.from_records(records, like, groups, 50)
    host = host_route(pkg, like, records, groups, 50)
    assert triple(built) == triple(host)
    return like, records, built, host


def test_index_properties(pkg, fifty):
    like, _, built, host = fifty
    assert built.has_abundances and built.max_hash == like.max_hash and len(built.nodes) == len(built) == 50
    assert built.sizes().tolist() == host.sizes().tolist()
    for a, b in zip(built.sketches(), host.sketches()):
        assert (a.ksize, a.molecule, a.seed, a.max_hash, a.num) == (b.ksize, b.molecule, b.seed, b.max_hash, b.num)
        assert a.mins == b.mins and a.abunds == b.abunds
    assert built.nodes[3].mins == host.nodes[3].mins
    assert not built.has_taxonomy


def test_downstream_calls_equal_the_host_built_index(pkg, fifty):
    like, records, built, host = fifty
    queries = host.nodes[:7]
    a, b = built.search_many(queries, 0.05), host.search_many(queries, 0.05)
    assert a.offsets.tolist() == b.offsets.tolist() and a.node.tolist() == b.node.tolist() and a.common.tolist() == b.common.tolist()
    ga, gb = built.gather(host.nodes[2]), host.gather(host.nodes[2])
    assert [r[:5] for r in ga.rows] == [r[:5] for r in gb.rows] and ga.assigned.tolist() == gb.assigned.tolist()
    grp = [g % 5 for g in range(50)]
    assert triple(built.collapse(grp, 5, abund="sum")) == triple(host.collapse(grp, 5, abund="sum"))
    ma, mb = built.match(records[:40], hits=True), host.match(records[:40], hits=True)
    for x, y in zip(ma, mb):
        assert x.tolist() == y.tolist()
    assert built.angular_matrix()["angular"].tolist() == host.angular_matrix()["angular"].tolist()


def test_records_handle_and_device_pointer_forms(pkg):
    import torch
    rng = np.random.default_rng(31)
    like = like_of(pkg, 21)
    seqs = [dna(rng, n) for n in (200, 50, 0, 120)]
    want = IB.build(seqs, [1, 0, 1, 1], 2, params(like))
    text = b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs))
    recs = pkg.fastx.Records.parse(text)
    assert len(recs) == 4
    assert triple(pkg.index.ResidentIndex.from_records(recs, like, [1, 0, 1, 1])) == want
    flat = torch.from_numpy(np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()).cuda()
    off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    torch.cuda.synchronize()
    assert triple(pkg.index.ResidentIndex.from_records((flat.data_ptr(), flat.numel(), off), like, [1, 0, 1, 1])) == want
    assert triple(pkg.index.ResidentIndex.from_records((flat.data_ptr(), flat.numel(), off), like)) == IB.build(seqs, None, 4, params(like))


def test_refusals_leave_nothing_behind(pkg):
    like = like_of(pkg, 21)
    R = pkg.index.ResidentIndex
    for args, kw in ((([b"ACGT" * 10], pkg.KmerMinHash(500, 21)), {}),
                     (([b"ACGT" * 10], like), dict(amino=True)),
                     (([b"ACGT" * 10], like, [3]), dict(n_groups=2)),
                     (([b"ACGT" * 10], like), dict(n_groups=2)),
                     (([b"ACGT" * 10], like, [0]), dict(n_groups=1 << 24))):
        with pytest.raises(pkg.SourmashError) as e:
            R.from_records(*args, **kw)
        assert e.value.code == 3
    with pytest.raises(pkg.SourmashError) as e:    # the translated arm's own error: a byte >= 0x80 that is not UTF-8
        R.from_records([b"ACGTACGTAC\xff\xfeGTACGTACGTACGTACGTACGTACG"], like_of(pkg, 21, "protein"))
    assert e.value.code == 1
    assert len(R.from_records([], like)) == 0 and len(R.from_records([b"ACGT"], like, [0], 1)) == 1


def test_concat(pkg, fifty):
    like, records, built, host = fifty
    R = pkg.index.ResidentIndex
    rng = np.random.default_rng(37)
    flat_like = like_of(pkg, 21, track=False, max_hash=like.max_hash)
    flat = R.from_records([dna(rng, 300), dna(rng, 100)], flat_like)
    cut = host.downsample(max_hash=like.max_hash // 3)
    before = count(pkg, "index_concat")
    # built here + host-built + a downsample() child; every part tracks abundances (the host part keeps them on the host)
    parts = [built, host, cut]
    joined = R.concat(parts)
    assert count(pkg, "index_concat") == before + 1
    assert triple(joined) == IB.concat([triple(p) for p in parts]) and joined.has_abundances and len(joined.nodes) == len(joined) == 150
    assert joined.max_hash is None and joined.max_hash_range == (like.max_hash // 3, like.max_hash)
    want = [s for p in parts for s in p.sketches()]
    for a, b in zip(joined.sketches(), want):
        assert (a.max_hash, a.ksize, a.mins, a.abunds) == (b.max_hash, b.ksize, b.mins, b.abunds)
    # a part whose abundances moved to HBM (an angular call), next to one that keeps them on the host
    host.norms2()
    again = R.concat([host, built, host_route(pkg, like, records[:6], [0, 0, 0, 1, 1, 1], 2)])
    assert triple(again) == IB.concat([triple(host), triple(built), triple(host_route(pkg, like, records[:6], [0, 0, 0, 1, 1, 1], 2))])
    assert again.norms2().tolist()[:50] == host.norms2().tolist()
    # with and without abundances -> none
    mixed = R.concat([built, flat])
    assert not mixed.has_abundances and triple(mixed) == IB.concat([triple(built), triple(flat)]) and triple(mixed)[2] is None
    # empty parts, zero parts, one part
    empty = R.from_records([], like)
    assert triple(R.concat([empty, flat, empty])) == triple(flat)
    assert triple(R.concat([])) == ([0], [], []) and len(R.concat([])) == 0
    assert triple(R.concat([built])) == triple(built)
    # the result equals the index of all the nodes for the calls downstream
    both = R.concat([built, built.collapse([g % 5 for g in range(50)], 5, abund="sum")])
    assert 4 in both.find(host.nodes[4], 0.99) and len(both) == 55
    assert triple(both.collapse([0] * 55, 1)) == triple(R(both.sketches()).collapse([0] * 55, 1))


def test_concat_with_a_num_index_among_scaled_ones(pkg, fifty):
    like, records, built, host = fifty
    nums = []
    for k in range(3):                                                  # bottom-20 sketches under the index's max_hash
        m = pkg.KmerMinHash(20, 21, False, 42, like.max_hash, False)
        m.add_sequence(records[k], True)
        nums.append(m)
    part = pkg.index.ResidentIndex(nums)
    joined = pkg.index.ResidentIndex.concat([part, built])
    whole = pkg.index.ResidentIndex(nums + host.sketches())
    assert triple(joined)[:2] == triple(whole)[:2] and len(joined) == 53 and not joined.has_abundances
    for q, thr in ((nums[1], 0.99), (nums[0], 0.0), (host.nodes[7], 0.2)):   # find still answers, as for the host-built mix
        found = joined.find(q, thr)
        assert found == whole.find(q, thr) and found
    assert 1 in joined.find(nums[1], 0.99)
    for idx in (joined, whole):                                         # refused as it would be for a host-built mix
        with pytest.raises(pkg.SourmashError) as e:
            idx.collapse([0] * 53, 1)
        assert e.value.code == 3 and "not a scaled sketch" in e.value.message


def test_parts_freed_before_the_result_is_used(pkg):
    rng = np.random.default_rng(41)
    like = like_of(pkg, 21)
    recs = [[dna(rng, 150), dna(rng, 80)] for _ in range(3)]
    parts = [pkg.index.ResidentIndex.from_records(r, like) for r in recs]
    want = IB.concat([triple(p) for p in parts])
    joined = pkg.index.ResidentIndex.concat(parts)
    del parts
    import gc
    gc.collect()
    pkg.lib().smh_release_workspace()
    assert triple(joined) == want
    assert [s.mins for s in joined.sketches()] == [want[1][want[0][v]:want[0][v + 1]] for v in range(6)]
