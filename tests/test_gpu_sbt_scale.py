"""SBT search on the device at the sizes and shapes where its branches change (reference src/index/sbt.rs:147-277,
src/index/nodegraph.rs): both leaf-walk paths at the LDS limit, query chunks with a full leaf-pair list, leaves of mixed
`num` at exact thresholds, tree shapes (arity, table counts, the node-table LDS limit), errors across chunks and leaf
classes, and the Nodegraph's batched forms over several grid-stride turns, all against the tests' restatement
(sbt_restatement.py).  Every result is exact, so every comparison is for equality, order included.

The two tests at the end pin the restatement's new helpers and need no GPU."""
import ctypes as C
import json
import math
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, sorted_sketch
import sbt_restatement as R

V5_SIZES = [99991, 99989, 99971, 99961]
LDS_BYTES = 64 * 1024        # k_sbt_nodes stages a node's tables, k_sbt_leaves a (leaf, query) pair, up to this size
GRID_THREADS = 4096 * 256    # sbt_grid's cap: the grid-stride kernels take a second turn beyond this many items
CHUNK_ENTRIES = 8 << 20      # Sbt::find_many: queries per chunk = 8 Mi / max(widest level of internal nodes, leaves)


def rand_hashes(rng, n, below=2**64 - 1):
    return rng.integers(1, below, n, dtype=np.uint64)


def sketch(pkg, mins, num=0, ksize=21, seed=42, max_hash=0):
    """a sketch holding exactly `mins` (ascending, distinct, all kept by num / max_hash)"""
    mh = pkg.KmerMinHash(num, ksize, False, seed, max_hash, False)
    mins = np.asarray(mins, dtype=np.uint64)
    mh.add_many(mins)
    assert len(mh) == mins.size
    return mh


def depth_of(pos, d):
    k = 0
    while pos:
        pos = (pos - 1) // d
        k += 1
    return k


def ancestors(d, positions):
    out = set()
    for pos in positions:
        while pos:
            pos = (pos - 1) // d
            out.add(pos)
    return out


def queries_per_chunk(d, positions, n_queries):
    widest = {}
    for p in ancestors(d, positions):
        widest[depth_of(p, d)] = widest.get(depth_of(p, d), 0) + 1
    per_query = max(max(widest.values(), default=1), len(positions), 1)
    return max(1, min(n_queries, CHUNK_ENTRIES // per_query))


class Profile:
    """the library's per-kernel launch counts (smh_profile_*) over a block"""

    def __init__(self, pkg):
        self.L = pkg.lib()

    def __enter__(self):
        self.L.smh_profile_reset()
        self.L.smh_profile_enable(1)
        return self

    def __exit__(self, *exc):
        self.L.smh_profile_enable(0)

    def launches(self, name):
        ms, n = C.c_double(), C.c_uint64()
        self.L.smh_profile_get(name.encode(), C.byref(ms), C.byref(n))
        return n.value


def raw_find_many(pkg, t, queries, threshold, containment):
    """smh_sbt_find_many called as SBT.find_many calls it, the results kept as numpy arrays (offsets, positions)"""
    L = pkg.lib()
    arr = (C.c_void_p * max(len(queries), 1))(*[q._p for q in queries])
    offs = np.zeros(len(queries) + 1, dtype=np.uint64)
    pos = C.POINTER(C.c_uint64)()
    pkg.errors.call(L.smh_sbt_find_many, t._p, arr, len(queries), float(threshold), bool(containment),
                    offs.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(pos))
    total = int(offs[-1])
    flat = np.ctypeslib.as_array(pos, shape=(total,)).copy() if total else np.zeros(0, dtype=np.uint64)
    return offs, flat


# ---------------------------------------------------------------------------------------------------------------------
# 1. the two leaf-walk paths of k_sbt_leaves on the same pairs, at their limit

@pytest.mark.gpu
def test_leaf_pairs_staged_and_global_agree_at_the_lds_limit(pkg):
    rng = np.random.default_rng(101)
    max_hash = 2**62
    pools = [rand_hashes(rng, 6000, max_hash) for _ in range(8)]
    lens = [0, 0, 4096, 4096, 1, 2, 63, 64, 65, 4095] + [int(x) for x in rng.integers(100, 4097, 30)]
    rng.shuffle(lens)
    leaf_mins = []
    for i, n in enumerate(lens):
        pool = pools[i * len(pools) // len(lens)]   # family order
        own = min(n, int(n * 0.8))
        leaf_mins.append(np.unique(np.concatenate([rng.choice(pool, own, replace=False),
                                                   rand_hashes(rng, n - own, max_hash)])))
    leaves = [sketch(pkg, m, max_hash=max_hash) for m in leaf_mins]
    positions = pkg.sbt.default_positions(len(leaves), 2)
    t = pkg.SBT.build(leaves, V5_SIZES, ksize=21, d=2, positions=positions)

    def mixed(n, fams):
        part = [rng.choice(pools[f], n // len(fams), replace=False) for f in fams]
        s = np.unique(np.concatenate(part + [rand_hashes(rng, n - sum(p.size for p in part), max_hash)]))
        assert s.size == n
        return s

    q_mins = [leaf_mins[i] for i in (lens.index(4096), lens.index(1), lens.index(65), 7, 21, 33)]
    q_mins += [np.zeros(0, dtype=np.uint64), mixed(4096, [0]), mixed(3000, [2, 3]), mixed(1, [5]), mixed(700, [7])]
    big = mixed(4097, [4, 5])
    batch = [sketch(pkg, m, max_hash=max_hash) for m in q_mins]
    batch_big = batch + [sketch(pkg, big, max_hash=max_hash)]
    # launch_sbt_leaves stages a pair when (longest leaf + longest query of the batch) * 8 bytes fit: exactly at the
    # limit for `batch`, one hash past it (every pair through global memory) for `batch_big`
    assert max(lens) == 4096 and max(m.size for m in q_mins) == 4096
    assert (max(lens) + 4096) * 8 == LDS_BYTES and (max(lens) + big.size) * 8 > LDS_BYTES

    nodes = R.build_nodes(2, {p: m.tolist() for p, m in zip(positions, leaf_mins)}, V5_SIZES)
    lv = {p: (m.tolist(), 0) for p, m in zip(positions, leaf_mins)}
    for thr in (-0.5, 0, 0.05, 0.3, 0.9):
        for cont in (False, True):
            staged = t.find_many(batch, thr, cont)
            gathered = t.find_many(batch_big, thr, cont)
            assert gathered[:len(batch)] == staged, (thr, cont)
            for qm, got in zip(q_mins + [big], gathered):
                assert got == R.find(2, V5_SIZES, nodes, lv, qm.tolist(), thr, cont), (thr, cont, qm.size)


# ---------------------------------------------------------------------------------------------------------------------
# 2 and 5. a tree wide enough that a batch walks in several query chunks

class ChunkTree:
    N_LEAVES, N_QUERIES, FAMILIES = 12000, 2500, 60

    def __init__(self, pkg):
        rng = np.random.default_rng(202)
        cores = [rand_hashes(rng, 400) for _ in range(self.FAMILIES)]
        self.leaf_mins = []
        for i in range(self.N_LEAVES):
            n = int(rng.integers(60, 201))
            own = min(n, int(rng.integers(40, 160)))
            core = cores[i * self.FAMILIES // self.N_LEAVES]   # family order
            self.leaf_mins.append(np.unique(np.concatenate([rng.choice(core, own, replace=False),
                                                            rand_hashes(rng, n - own)])))
        self.leaves = [sketch(pkg, m, num=200) for m in self.leaf_mins]
        self.positions = pkg.sbt.default_positions(self.N_LEAVES, 2)
        self.t = pkg.SBT.build(self.leaves, V5_SIZES, ksize=21, d=2, positions=self.positions)
        # leaf queries, and every 25th query a large one: a family core and 7 600 hashes of no leaf, so that the batch
        # holds more query hashes than one grid-stride turn of k_sbt_bins covers
        self.big_at = set(range(12, self.N_QUERIES, 25))
        self.query_mins, self.queries = [], []
        for i in range(self.N_QUERIES):
            if i in self.big_at:
                m = np.unique(np.concatenate([cores[int(rng.integers(self.FAMILIES))], rand_hashes(rng, 7600)]))
                self.query_mins.append(m)
                self.queries.append(sketch(pkg, m, num=8000))
            else:
                j = int(rng.integers(self.N_LEAVES))
                self.query_mins.append(self.leaf_mins[j])
                self.queries.append(self.leaves[j])
        self.chunk = queries_per_chunk(2, self.positions, self.N_QUERIES)
        self.nodes = R.LazyNodes(2, dict(zip(self.positions, self.leaf_mins)), V5_SIZES)
        self.lv = {p: (m.tolist(), 200) for p, m in zip(self.positions, self.leaf_mins)}

    def restated(self, qm, thr, cont, codes=None):
        return R.find(2, V5_SIZES, self.nodes, self.lv, qm.tolist(), thr, cont, codes)


@pytest.fixture(scope="module")
def chunk_tree(pkg):
    return ChunkTree(pkg)


@pytest.mark.gpu
def test_query_chunks_and_the_full_leaf_pair_list(pkg, chunk_tree):
    ct = chunk_tree
    n_levels = depth_of(ct.positions[-1], 2)
    assert sum(m.size for m in ct.query_mins) > GRID_THREADS       # k_sbt_bins: a second grid-stride turn
    chunks = [(c0, min(c0 + ct.chunk, ct.N_QUERIES)) for c0 in range(0, ct.N_QUERIES, ct.chunk)]
    assert len(chunks) >= 3
    sample = sorted({i for c0, c1 in chunks for i in (c0, c1 - 1)} | {12, 1412, 300, 1800})   # 12, 1412: large
    for cont in (False, True):
        with Profile(pkg) as prof:
            many = ct.t.find_many(ct.queries, 0.1, cont)
            # one k_sbt_leaves launch per chunk, one k_sbt_nodes launch per level and chunk, k_sbt_bins once
            assert prof.launches("sbt_leaves") == len(chunks)
            assert prof.launches("sbt_nodes") == len(chunks) * n_levels
            assert prof.launches("sbt_bins") == 1
        assert sum(map(len, many)) > ct.N_QUERIES, cont
        for i in sample:
            assert many[i] == ct.restated(ct.query_mins[i], 0.1, cont), (cont, i)
        if not cont:
            for i, q in enumerate(ct.queries):
                assert many[i] == ct.t.find_positions(q, 0.1, False), i

    # threshold -1 (similarity, no empty leaf): every node and every leaf passes, so each query's answer is every leaf
    # in the walk's order, and each chunk's leaf-pair list holds exactly its capacity, chunk size x leaves
    assert min(m.size for m in ct.leaf_mins) > 0
    order = np.array(R.walk_order(2, ct.positions), dtype=np.uint64)
    assert sorted(order.tolist()) == ct.positions
    small = [q for i, q in enumerate(ct.queries) if i not in ct.big_at][:2 * ct.chunk + 100]
    with Profile(pkg) as prof:
        offs, flat = raw_find_many(pkg, ct.t, small, -1, False)
        assert prof.launches("sbt_leaves") == 3
    assert np.array_equal(np.diff(offs), np.full(len(small), ct.N_LEAVES, dtype=np.uint64))
    assert np.array_equal(flat.reshape(len(small), ct.N_LEAVES), np.broadcast_to(order, (len(small), ct.N_LEAVES)))


@pytest.mark.gpu
def test_errors_across_chunks(pkg, chunk_tree):
    ct = chunk_tree
    base = ct.t.find_many(ct.queries, 0.1, False)
    in2, in3 = ct.chunk + 5, 2 * ct.chunk + 7      # a query of chunk 2 and one of chunk 3
    assert in2 // ct.chunk == 1 and in3 // ct.chunk == 2 and in2 not in ct.big_at and in3 not in ct.big_at
    other_k = sketch(pkg, ct.query_mins[in2], num=200, ksize=31)
    other_seed = sketch(pkg, ct.query_mins[in3], num=200, seed=7)
    # both walks reach leaves (every leaf is k = 21, seed 42): the lowest query index decides the error
    codes_all = {p: 1 for p in ct.positions}
    for i in (in2, in3):
        with pytest.raises(R.Incompatible):
            ct.restated(ct.query_mins[i], 0.1, False, codes_all)
    for a, b, code in ((other_k, other_seed, 101), (other_seed, other_k, 104)):
        batch = list(ct.queries)
        batch[in2], batch[in3] = a, b
        with pytest.raises(pkg.SourmashError) as ei:
            ct.t.find_many(batch, 0.1, False)
        assert ei.value.code == code
    # an incompatible query whose walk passes the top of the tree but reaches no leaf raises nothing
    rng = np.random.default_rng(5)
    stray_mins = rand_hashes(rng, 150)
    stray_mins.sort()
    assert ct.restated(stray_mins, 0.1, False, codes_all) == []
    tables, mnb = ct.nodes[0]
    assert R.matches(V5_SIZES, tables, stray_mins.tolist()) / mnb > 0.1    # the root passes
    batch = list(ct.queries)
    batch[in3] = sketch(pkg, stray_mins, num=200, ksize=31)
    got = ct.t.find_many(batch, 0.1, False)
    assert got[in3] == [] and got[:in3] == base[:in3] and got[in3 + 1:] == base[in3 + 1:]


@pytest.mark.gpu
def test_mixed_leaf_classes_raise_the_first_reached_leafs_code(pkg):
    rng = np.random.default_rng(505)
    fams = [rand_hashes(rng, 600) for _ in range(5)]
    positions = pkg.sbt.default_positions(64, 2)   # 63 .. 126: the left subtree holds 63 .. 94
    # left: k = 21 (families 0, 1); right: 95 .. 102 k = 21 seed 7 (family 2), 103 .. 126 k = 31 (families 3, 4)
    params, fam_of = {}, {}
    for i, p in enumerate(positions):
        if i < 32:
            params[p], fam_of[p] = (21, 42), i // 16
        elif i < 40:
            params[p], fam_of[p] = (21, 7), 2
        else:
            params[p], fam_of[p] = (31, 42), 3 + (i - 40) // 12
    leaf_mins = {}
    for p in positions:
        n = int(rng.integers(80, 201))
        own = int(n * 0.7)
        leaf_mins[p] = np.unique(np.concatenate([rng.choice(fams[fam_of[p]], own, replace=False),
                                                 rand_hashes(rng, n - own)]))
    leaves = [sketch(pkg, leaf_mins[p], num=200, ksize=params[p][0], seed=params[p][1]) for p in positions]
    t = pkg.SBT.build(leaves, V5_SIZES, ksize=21, d=2, positions=positions)
    nodes = R.build_nodes(2, {p: m.tolist() for p, m in leaf_mins.items()}, V5_SIZES)
    lv = {p: (m.tolist(), 200) for p, m in leaf_mins.items()}
    codes = {p: R.check_code((params[p][0], False, 0, params[p][1]), (21, False, 0, 42)) for p in positions}
    q_mins = [leaf_mins[70],                                                              # family 0: stays left
              np.unique(np.concatenate([leaf_mins[85], rng.choice(fams[2], 150, replace=False)])),   # 1 and 2
              np.unique(np.concatenate([leaf_mins[66], rng.choice(fams[4], 20, replace=False)]))]    # 0, a little of 4
    raised, found = set(), 0
    for qm in q_mins:
        q = sketch(pkg, qm, num=400)
        for thr in (-0.5, 0, 0.05, 0.2, 0.5, 0.9):
            for cont in (False, True):
                try:
                    want = R.find(2, V5_SIZES, nodes, lv, qm.tolist(), thr, cont, codes)
                except R.Incompatible as e:
                    with pytest.raises(pkg.SourmashError) as ei:
                        t.find_many([q], thr, cont)
                    assert ei.value.code == e.code, (thr, cont, e.pos)
                    raised.add(e.code)
                    continue
                assert t.find_many([q], thr, cont) == [want], (thr, cont)
                found += len(want) > 0
    # the cases reach both incompatible classes first, and some walks stay among the compatible leaves and find hits
    assert raised == {101, 104} and found >= 3


# ---------------------------------------------------------------------------------------------------------------------
# 3. leaves of mixed num; thresholds equal to a leaf's exact value

@pytest.mark.gpu
def test_mixed_num_leaves_and_exact_thresholds(pkg):
    rng = np.random.default_rng(303)
    pools = [rand_hashes(rng, 6000) for _ in range(4)]

    def member(fams):
        keep = [p[rng.random(p.size) < 0.7] for p in (pools[f] for f in fams)]
        return np.unique(np.concatenate(keep + [rand_hashes(rng, 500)]))

    nums = (10, 50, 300, 2000)
    positions = pkg.sbt.default_positions(64, 2)
    leaf_mins = {p: member([i // 16])[:nums[i % 4]] for i, p in enumerate(positions)}
    leaf_num = {p: nums[i % 4] for i, p in enumerate(positions)}
    t = pkg.SBT.build([sketch(pkg, leaf_mins[p], num=leaf_num[p]) for p in positions], V5_SIZES, ksize=21, d=2,
                      positions=positions)
    q_nums = (20, 100, 500, 3000)
    q_mins = [member([j % 4] if j < 8 else [j % 4, (j + 1) % 4])[:q_nums[j % 4]] for j in range(12)]
    queries = [sketch(pkg, m, num=q_nums[j % 4]) for j, m in enumerate(q_mins)]
    nodes = R.build_nodes(2, {p: m.tolist() for p, m in leaf_mins.items()}, V5_SIZES)
    lv = {p: (m.tolist(), leaf_num[p]) for p, m in leaf_mins.items()}

    def want(j, thr, cont):
        return R.find(2, V5_SIZES, nodes, lv, q_mins[j].tolist(), thr, cont)

    for thr in (-0.5, 0, 0.1, 0.3, 0.6):
        for cont in (False, True):
            for j, got in enumerate(t.find_many(queries, thr, cont)):
                assert got == want(j, thr, cont), (thr, cont, j)

    # (leaf, query) pairs at the leaf's exact value: absent at that threshold (value > threshold), present just below
    pairs = [(j, p) for j in range(len(queries)) for p in positions]
    random.Random(7).shuffle(pairs)
    for cont in (False, True):
        per_num, chosen = {}, []
        for j, p in pairs:
            lm, qm = lv[p][0], q_mins[j].tolist()
            if cont:
                value = len(set(lm) & set(qm)) / len(lm)
            else:
                value = R.compare(lm, qm, leaf_num[p])
                if len(set(lm) | set(qm)) <= leaf_num[p]:
                    continue              # the leaf's num does not truncate this union
            if not 0 < value or per_num.get(leaf_num[p], 0) >= 2:
                continue
            below = math.nextafter(value, -math.inf)
            if p not in want(j, below, cont):
                continue                  # the walk does not reach the leaf
            per_num[leaf_num[p]] = per_num.get(leaf_num[p], 0) + 1
            chosen.append((j, p, value, below))
        assert len(chosen) >= 6 and len(per_num) == 4, (cont, per_num)
        for j, p, value, below in chosen:
            at, under = want(j, value, cont), want(j, below, cont)
            assert p not in at and p in under
            assert t.find_many([queries[j]], value, cont) == [at], (cont, j, p, value)
            assert t.find_many([queries[j]], below, cont) == [under], (cont, j, p, below)


# ---------------------------------------------------------------------------------------------------------------------
# 4. tree shapes: arity, leaves of mixed depth, 1 / 2 / 6 tables, the node-table LDS limit

def random_positions(rng, d, n, max_depth):
    """up to n leaf positions of depth 2 .. max_depth in a d-ary tree, no leaf an ancestor of another"""
    leaves, above = set(), set()
    for _ in range(200 * n):
        if len(leaves) == n:
            break
        depth = rng.randint(2, max_depth)
        pos = (d ** depth - 1) // (d - 1) + rng.randrange(d ** depth)
        up = ancestors(d, [pos])
        if pos in leaves or pos in above or up & leaves:
            continue
        leaves.add(pos)
        above |= up
    return sorted(leaves)


SHAPES = [
    (2, 8, [1021]),
    (3, 6, [251, 257]),
    (4, 5, [61, 67, 71, 73, 79, 83]),
    (5, 4, [4093, 4091]),
    (8, 4, [509, 503, 499, 491, 487, 479]),
    (8, 3, [127]),
    (2, 7, [131071, 131063, 131059, 131072]),   # 8 192 words = 64 KiB: k_sbt_nodes stages the tables in LDS
    (4, 5, [131071, 131063, 131059, 131073]),   # 8 193 words: read from global memory
]


@pytest.mark.gpu
@pytest.mark.parametrize("d,max_depth,sizes", SHAPES)
def test_tree_shapes_match_the_restatement(pkg, tmp_path, d, max_depth, sizes):
    rng = random.Random(d * 100 + len(sizes) * 10 + max_depth)
    nrng = np.random.default_rng(d * 100 + len(sizes))
    positions = random_positions(rng, d, 32, max_depth)
    assert len(positions) == 32 and len({depth_of(p, d) for p in positions}) >= 2
    internal = ancestors(d, positions)
    slots = {d * p + c + 1 for p in internal for c in range(d)}
    assert slots - internal - set(positions)          # some child slots are empty
    if sizes[0] == 131071:
        words = sum((s + 63) // 64 for s in sizes)
        assert (words * 8 <= LDS_BYTES) == (sizes[-1] == 131072)
    fams = [rand_hashes(nrng, 500) for _ in range(4)]
    leaf_mins = {}
    for k, p in enumerate(positions):
        n = 0 if k == 3 else int(nrng.integers(1, 301))
        own = int(n * 0.6)
        leaf_mins[p] = np.unique(np.concatenate([nrng.choice(fams[rng.randrange(4)], own, replace=False),
                                                 rand_hashes(nrng, n - own)]))
    t = pkg.SBT.build([sketch(pkg, leaf_mins[p], num=300) for p in positions], sizes, ksize=21, d=d,
                      positions=positions)
    lm = {p: m.tolist() for p, m in leaf_mins.items()}
    nodes = R.build_nodes(d, lm, sizes)
    assert set(nodes) == internal

    t.save(tmp_path / "shape.sbt.json")
    saved = json.load(open(tmp_path / "shape.sbt.json"))
    assert saved["d"] == d and {int(p) for p in saved["nodes"]} == internal
    for p, v in saved["nodes"].items():
        ksize, occ, got_sizes, tables = R.load_nodegraph((tmp_path / ".sbt.shape" / v["filename"]).read_bytes())
        want_tables, mnb = nodes[int(p)]
        assert got_sizes == sizes and ksize == 21
        assert all(np.array_equal(a, b) for a, b in zip(tables, want_tables)), p
        assert occ == int(want_tables[0].sum())
        assert v["metadata"]["min_n_below"] == mnb
    if max(sizes) < 2000:
        assert min(tb.mean() for tb in nodes[0][0]) > 0.9      # small tables: the root's filters are saturated

    lv = {p: (lm[p], 300) for p in positions}
    q_mins = [leaf_mins[p] for p in rng.sample(positions, 8)]
    q_mins += [np.zeros(0, dtype=np.uint64), np.unique(np.concatenate([fams[0][:150], fams[1][:150]]))]
    queries = [sketch(pkg, m, num=300) for m in q_mins]
    for thr in (-0.5, 0, 0.1, 0.4, 0.8):
        for cont in (False, True):
            for qm, got in zip(q_mins, t.find_many(queries, thr, cont)):
                assert got == R.find(d, sizes, nodes, lv, qm.tolist(), thr, cont), (thr, cont)


# ---------------------------------------------------------------------------------------------------------------------
# 6. Nodegraph count_many / get_many over several grid-stride turns

# four tables the batches below fill up, one that saturates within the first turn, and three large enough that they
# keep clear bits (get_many answers both ways there)
NG_SIZES = [[99991, 99989, 99971, 99961], [1000], [4194301, 4194287, 4194277]]


def ng_batch(rng, sizes, n):
    """n hashes, shuffled: a third uniform, a third exact repeats of those, a third distinct hashes that share bins with
    them (a multiple of one table's size apart, or of the product of two sizes)"""
    k = n // 3
    uni = np.concatenate([rng.integers(0, 2**63, k - 2, dtype=np.uint64), np.array([0, 2**64 - 1], dtype=np.uint64)])
    rep = uni[rng.integers(0, k, k)]
    m = n - 2 * k
    s = np.array(sizes, dtype=np.uint64)
    ti = rng.integers(0, len(sizes), m)
    step = s[ti]
    if len(sizes) > 1:
        two = rng.random(m) < 0.3
        step[two] *= s[(ti[two] + 1) % len(sizes)]
    base = uni[rng.integers(0, k - 1, m)]     # not 2^64 - 1
    share = base + step * rng.integers(1, 1 << 20, m, dtype=np.uint64)
    out = np.concatenate([uni, rep, share])
    rng.shuffle(out)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", NG_SIZES)
def test_count_many_and_get_many_at_scale(pkg, sizes):
    rng = np.random.default_rng(606 + len(sizes))
    ng = pkg.Nodegraph(sizes, 21)
    tables = [np.zeros(s, dtype=bool) for s in sizes]
    occupied = unique = 0
    first = ng_batch(rng, sizes, 3_000_000)
    second = np.concatenate([ng_batch(rng, sizes, 1_000_000), first[rng.integers(0, first.size, 500_000)]])
    rng.shuffle(second)
    for k, batch in enumerate((first, second)):
        got = ng.count_many(batch)
        new, bits, kmers = R.count_many(sizes, tables, batch)
        occupied += bits
        unique += kmers
        assert np.array_equal(got, new), k
        assert (ng.n_occupied_bins(), ng.unique_kmers()) == (occupied, unique), k
        assert ng.to_bytes() == R.nodegraph_bytes(21, occupied, sizes, tables), k
        if k == 0:
            assert new.any() and not new.all()
            if len(sizes) > 1:
                assert new[GRID_THREADS:].any()      # bins first set in the grid-stride loops' second turn
    probe = np.concatenate([rng.integers(0, 2**64 - 1, 2_000_000, dtype=np.uint64),
                            second[rng.integers(0, second.size, 1_000_000)]])
    rng.shuffle(probe)
    want = R.get_many(sizes, tables, probe)
    if sizes == NG_SIZES[2]:
        assert 0.1 < want.mean() < 0.9
    assert np.array_equal(ng.get_many(probe).astype(bool), want)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement's new helpers, pinned on the host

@pytest.mark.parametrize("sizes", NG_SIZES)
def test_count_restatement_matches_host_count(pkg, sizes):
    rng = np.random.default_rng(707 + len(sizes))
    hashes = ng_batch(rng, sizes, 50_000)
    ng = pkg.Nodegraph(sizes, 21)
    tables = [np.zeros(s, dtype=bool) for s in sizes]
    occupied = unique = 0
    for part in (hashes[:30_000], hashes[30_000:]):      # the second part sees the first part's bits
        flags = [ng.count(int(h)) for h in part]
        new, bits, kmers = R.count_many(sizes, tables, part)
        occupied += bits
        unique += kmers
        assert flags == new.tolist()
        assert (ng.n_occupied_bins(), ng.unique_kmers()) == (occupied, unique)
        assert ng.to_bytes() == R.nodegraph_bytes(21, occupied, sizes, tables)
    probe = np.concatenate([rng.integers(0, 2**64 - 1, 3000, dtype=np.uint64), hashes[:3000]])
    assert [ng.get(int(h)) == 1 for h in probe] == R.get_many(sizes, tables, probe).tolist()


def test_walk_order_lazy_nodes_and_check_code_match_the_restatement(pkg):
    # v5: the reference's own node files
    tree = json.load(open(os.path.join(GOLDEN, "v5.sbt.json")))
    nodes, leaves, sizes = {}, {}, None
    for p, v in tree["nodes"].items():
        _, _, sizes, tables = R.load_nodegraph(open(os.path.join(GOLDEN, "sbt_v5", v["filename"]), "rb").read())
        nodes[int(p)] = (tables, v["metadata"]["min_n_below"])
    for p, v in tree["leaves"].items():
        sk = json.load(open(os.path.join(GOLDEN, "sbt_v5", v["filename"] + ".sig")))[0]["signatures"][0]
        leaves[int(p)] = (sorted(sk["mins"]), sk["num"])
    order = R.walk_order(tree["d"], sorted(leaves))
    assert sorted(order) == sorted(leaves)
    for q in leaves:
        for cont in (False, True):
            assert R.find(tree["d"], sizes, nodes, leaves, leaves[q][0], -1, cont) == order
    # subset: nodes built from the leaves, whole and lazily
    import gzip
    sub = json.load(open(os.path.join(GOLDEN, "subset.sbt.json")))
    with gzip.open(os.path.join(GOLDEN, "sbt_subset_sigs.json.gz"), "rt") as fh:
        sigs = json.load(fh)
    leaves = {}
    for p, v in sub["leaves"].items():
        sk = sorted_sketch(sigs[v["filename"]][0]["signatures"][0])
        leaves[int(p)] = (sk["mins"], 0 if sk["max_hash"] else sk["num"])
    built = R.build_nodes(sub["d"], {p: m for p, (m, _) in leaves.items()}, V5_SIZES)
    lazy = R.LazyNodes(sub["d"], {p: m for p, (m, _) in leaves.items()}, V5_SIZES, keep=8)
    assert set(lazy.below) == set(built) and all(p in lazy for p in built)
    for p, (tables, mnb) in built.items():
        lt, lm = lazy[p]
        assert lm == mnb and all(np.array_equal(a, b) for a, b in zip(lt, tables)), p
    order = R.walk_order(sub["d"], sorted(leaves))
    for q in sorted(leaves)[::33]:
        assert R.find(sub["d"], V5_SIZES, built, leaves, leaves[q][0], -1, False) == order
        for thr in (0.05, 0.3):
            assert R.find(sub["d"], V5_SIZES, lazy, leaves, leaves[q][0], thr, True) == \
                R.find(sub["d"], V5_SIZES, built, leaves, leaves[q][0], thr, True)
    # check_code is leaf.check_compatible(query)'s error code
    combos = [(21, False, 0, 42), (31, False, 0, 42), (21, True, 0, 42), (21, False, 1000, 42), (21, False, 0, 7),
              (31, True, 1000, 7), (21, False, 1000, 7)]
    for a in combos:
        for b in combos:
            ma, mb = (pkg.KmerMinHash(0 if x[2] else 500, x[0], x[1], x[3], x[2]) for x in (a, b))
            try:
                ma.check_compatible(mb)
                code = 0
            except pkg.SourmashError as e:
                code = e.code
            assert R.check_code(a, b) == code, (a, b)
