"""SBT search on the device (reference src/index/sbt.rs:147-277 with src/index/search.rs): the reference's trees, the
device build, the Nodegraph's batched forms and synthetic trees against the tests' restatement (sbt_restatement.py)."""
import gzip
import hashlib
import json
import os
import random
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, sorted_sketch
import sbt_restatement as R

pytestmark = pytest.mark.gpu

V5_SIZES = [99991, 99989, 99971, 99961]
THRESHOLDS = [0, 0.05, 0.1, 0.3, 0.5, 0.9, 1.0]


def mh_from_sketch(pkg, sk):
    mh = pkg.KmerMinHash(0 if sk["max_hash"] else sk["num"], sk["ksize"], sk["molecule"] == "protein", sk["seed"],
                         sk["max_hash"], False)
    for m in sk["mins"]:
        mh.mins_push(m)
    return mh


def v5_dir(tmp_path):
    """the reference's layout: v5.sbt.json + .sbt.v5/{leaf files, internal.N}"""
    tree = json.load(open(os.path.join(GOLDEN, "v5.sbt.json")))
    st = tmp_path / ".sbt.v5"
    st.mkdir()
    for v in tree["leaves"].values():
        shutil.copyfile(os.path.join(GOLDEN, "sbt_v5", v["filename"] + ".sig"), st / v["filename"])
    for v in tree["nodes"].values():
        shutil.copyfile(os.path.join(GOLDEN, "sbt_v5", v["filename"]), st / v["filename"])
    shutil.copyfile(os.path.join(GOLDEN, "v5.sbt.json"), tmp_path / "v5.sbt.json")
    return tmp_path / "v5.sbt.json", tree


def v5_leaves(pkg, tree):
    out = {}
    for p, v in tree["leaves"].items():
        sk = json.load(open(os.path.join(GOLDEN, "sbt_v5", v["filename"] + ".sig")))[0]["signatures"][0]
        out[int(p)] = mh_from_sketch(pkg, sorted_sketch(sk))
    return out


def subset_leaves(pkg):
    tree = json.load(open(os.path.join(GOLDEN, "subset.sbt.json")))
    with gzip.open(os.path.join(GOLDEN, "sbt_subset_sigs.json.gz"), "rt") as fh:
        sigs = json.load(fh)
    return tree, {int(p): mh_from_sketch(pkg, sorted_sketch(sigs[v["filename"]][0]["signatures"][0]))
                  for p, v in tree["leaves"].items()}


def expected(tag):
    return json.load(open(os.path.join(GOLDEN, "sbt_find_expected.json")))[tag]


def check_expected(pkg, t, leaves, tag):
    exp = expected(tag)
    for e in exp:
        if e["query"] % 7 == 0 or tag == "v5":   # per-query find on a sample; find_many on all of them below
            fn = pkg.index.search_minhashes_containment if e["containment"] else pkg.index.search_minhashes
            got = [leaf.pos for leaf in t.find(fn, leaves[e["query"]], e["threshold"])]
            assert got == e["hits"], e
    qpos = sorted(leaves)
    for thr in THRESHOLDS:
        for cont in (False, True):
            many = t.find_many([leaves[p] for p in qpos], thr, cont)
            want = {e["query"]: e["hits"] for e in exp if e["threshold"] == thr and e["containment"] == cont}
            assert {p: h for p, h in zip(qpos, many)} == want, (thr, cont)


def test_load_sbt_and_recorded_results(pkg, tmp_path):
    path, tree = v5_dir(tmp_path)
    t = pkg.SBT.from_path(path)
    assert t.n_nodes == 6 and len(t) == 7
    leaves = v5_leaves(pkg, tree)
    # reference sbt.rs:539-565 (load_sbt): leaf 7 as the query
    assert len(t.find(pkg.index.search_minhashes, leaves[7], 0.5)) == 1
    assert len(t.find(pkg.index.search_minhashes, leaves[7], 0.1)) == 2
    check_expected(pkg, t, leaves, "v5")
    assert sorted(t.leaf_positions()) == sorted(leaves)
    assert [lf.minhash.mins for lf in t.leaves()][0] == leaves[t.leaf_positions()[0]].mins


def test_build_v5_reproduces_the_reference_files(pkg, tmp_path):
    (tmp_path / "ref").mkdir()
    _, tree = v5_dir(tmp_path / "ref")
    leaves = v5_leaves(pkg, tree)
    pos = sorted(leaves)
    t = pkg.SBT.build([leaves[p] for p in pos], V5_SIZES, ksize=1, d=2, positions=pos)
    assert t.n_nodes == 6
    t.save(tmp_path / "built.sbt.json")
    for i in range(6):
        got = (tmp_path / ".sbt.built" / ("internal.%d" % i)).read_bytes()
        assert got == open(os.path.join(GOLDEN, "sbt_v5", "internal.%d" % i), "rb").read(), i
    # load(save(t)) finds what t finds
    t2 = pkg.SBT.from_path(tmp_path / "built.sbt.json")
    check_expected(pkg, t2, leaves, "v5")


def test_build_subset_matches_recorded_nodes_and_results(pkg, tmp_path):
    tree, leaves = subset_leaves(pkg)
    pos = sorted(leaves)
    t = pkg.SBT.build([leaves[p] for p in pos], V5_SIZES, ksize=1, d=tree["d"], positions=pos)
    assert t.n_nodes == 99
    t.save(tmp_path / "subset.sbt.json")
    rec = json.load(open(os.path.join(GOLDEN, "sbt_subset_nodes.json")))
    saved = json.load(open(tmp_path / "subset.sbt.json"))
    for p, r in rec.items():
        _, occ, sizes, tables = R.load_nodegraph((tmp_path / ".sbt.subset" / ("internal." + p)).read_bytes())
        assert hashlib.sha256(R.table_bytes(tables)).hexdigest() == r["sha256"], p
        assert [int(x.sum()) for x in tables] == r["popcounts"]
        assert saved["nodes"][p]["metadata"]["min_n_below"] == r["min_n_below"]
        assert occ == r["popcounts"][0]
    check_expected(pkg, t, leaves, "subset")


def test_count_many_get_many_match_host(pkg):
    rng = random.Random(11)
    for sizes in ([10], [7, 11]):
        hashes = [rng.choice([rng.getrandbits(64), rng.randrange(40)]) for _ in range(300)]
        host, dev = pkg.Nodegraph(sizes, 3), pkg.Nodegraph(sizes, 3)
        host.count(5)
        dev.count(5)
        new_host = [host.count(h) for h in hashes]
        new_dev = dev.count_many(hashes)
        assert list(new_dev) == new_host
        assert (dev.n_occupied_bins(), dev.unique_kmers()) == (host.n_occupied_bins(), host.unique_kmers())
        assert dev.to_bytes() == host.to_bytes()
        probe = [rng.getrandbits(64) for _ in range(200)] + hashes
        assert list(dev.get_many(probe)) == [host.get(h) for h in probe]
    # a bigger one against the reference's own node
    ng = pkg.Nodegraph.from_buffer(open(os.path.join(GOLDEN, "sbt_v5", "internal.0"), "rb").read())
    probe = [rng.getrandbits(64) for _ in range(2000)] + [801084876663808, 1877811740]
    assert list(ng.get_many(probe)) == [ng.get(h) for h in probe]


def test_device_modulo_is_exact(pkg):
    rng = random.Random(3)
    sizes = [1, 2, 3, 8, 10, 99991, 2**31 - 1, 2**32 - 5, rng.randrange(1, 2**32), rng.randrange(1, 2**16)]
    for s in sizes:
        hs = {0, 1, 2**64 - 1}
        for k in (1, 2, 3, 2**20 + 7, (2**64 - 1) // s - 1, (2**64 - 1) // s):
            for e in (-1, 0, 1):
                v = k * s + e
                if 0 <= v < 2**64:
                    hs.add(v)
        hs |= {rng.getrandbits(64) for _ in range(500)}
        hs = sorted(hs)
        got = pkg.sbt.device_bins([s], hs)[:, 0]
        assert [int(x) for x in got] == [h % s for h in hs], s
    hs = [rng.getrandbits(64) for _ in range(1000)]
    got = pkg.sbt.device_bins(sizes, hs)
    assert [[int(x) for x in row] for row in got] == [[h % s for s in sizes] for h in hs]


def family_leaves(pkg, rng, n, scaled, families=20):
    """family-structured sketches: members share much of a family core, ragged sizes"""
    cores = [[rng.getrandbits(64) >> (4 if scaled else 0) for _ in range(600)] for _ in range(families)]
    out = []
    for i in range(n):
        core = cores[i % families]
        keep = rng.randrange(50, 600)
        mins = set(rng.sample(core, keep)) | {rng.getrandbits(64) >> (4 if scaled else 0) for _ in range(rng.randrange(0, 200))}
        mins = sorted(mins)
        if scaled:
            mh = pkg.KmerMinHash(0, 21, False, 42, 2**60, False)
        else:
            mh = pkg.KmerMinHash(300, 21, False, 42, 0, False)
            mins = mins[:300]
        mh.add_many(np.array(mins, dtype=np.uint64))
        out.append(mh)
    return out


def restated(d, sizes, positions, leaves, num_of):
    lm = {p: list(mh.mins) for p, mh in zip(positions, leaves)}
    nodes = R.build_nodes(d, lm, sizes)
    return nodes, {p: (lm[p], num_of(mh)) for p, mh in zip(positions, leaves)}


@pytest.mark.parametrize("d,n,scaled,sizes", [
    (2, 600, False, [1009, 1013, 1019]),
    (3, 700, True, [99991, 99989, 99971, 99961]),
    (2, 500, False, [2097143, 2097133, 2097131, 2097091]),   # 1 MB of tables per node: the global-memory path
])
def test_synthetic_trees_match_restatement(pkg, d, n, scaled, sizes):
    rng = random.Random(d * 1000 + n)
    leaves = family_leaves(pkg, rng, n, scaled)
    leaves[5] = pkg.KmerMinHash(0, 21, False, 42, 2**60, False) if scaled else pkg.KmerMinHash(300, 21, False, 42, 0, False)
    positions = pkg.sbt.default_positions(n, d)
    t = pkg.SBT.build(leaves, sizes, ksize=21, d=d, positions=positions)
    nodes, lv = restated(d, sizes, positions, leaves, lambda mh: mh.num)
    queries = [leaves[i] for i in range(0, n, max(1, n // 40))] + [leaves[5]]
    for thr in (-0.5, 0, 0.1, 0.3, 0.8):
        for cont in (False, True):
            many = t.find_many(queries, thr, cont)
            for q, got in zip(queries, many):
                assert got == R.find(d, sizes, nodes, lv, list(q.mins), thr, cont), (thr, cont)


def test_missing_child_and_exact_ratio_threshold(pkg):
    rng = random.Random(9)
    leaves = family_leaves(pkg, rng, 40, False, families=4)
    positions = [p for i, p in enumerate(pkg.sbt.default_positions(64, 2)) if i % 3 != 1][:40]   # holes: missing children
    sizes = [1009, 1013]
    t = pkg.SBT.build(leaves, sizes, ksize=21, d=2, positions=positions)
    nodes, lv = restated(2, sizes, positions, leaves, lambda mh: mh.num)
    q = leaves[3]
    # a threshold equal to the root's exact ratio: the root does not pass (value > threshold), so nothing is found
    tables, mnb = nodes[0]
    ratio = R.matches(sizes, tables, list(q.mins)) / mnb
    assert t.find_many([q], ratio, False) == [[]]
    assert R.find(2, sizes, nodes, lv, list(q.mins), ratio, False) == []
    for thr in (0.0, 0.2, ratio - 1e-9):
        assert t.find_many([q], thr, False)[0] == R.find(2, sizes, nodes, lv, list(q.mins), thr, False)


def test_find_many_equals_find(pkg):
    rng = random.Random(21)
    leaves = family_leaves(pkg, rng, 1200, False, families=30)
    t = pkg.SBT.build(leaves, [4099, 4111, 4127, 4129], ksize=21, d=2)
    queries = [leaves[rng.randrange(len(leaves))] for _ in range(1000)]
    many = t.find_many(queries, 0.1, False)
    for i in range(0, 1000, 37):
        assert many[i] == t.find_positions(queries[i], 0.1, False)
    assert sum(len(x) for x in many) > 0


def test_errors_and_edges(pkg, tmp_path):
    path, tree = v5_dir(tmp_path)
    t = pkg.SBT.from_path(path)
    leaves = v5_leaves(pkg, tree)
    other_k = pkg.KmerMinHash(500, 21)
    for h in leaves[7].mins:
        other_k.mins_push(h)
    with pytest.raises(pkg.SourmashError) as ei:
        t.find(pkg.index.search_minhashes, other_k, 0.1)
    assert ei.value.code == 101
    # a query that reaches no leaf raises nothing (empty query: value 0.0 at the root)
    assert t.find(pkg.index.search_minhashes, pkg.KmerMinHash(500, 21), 0.1) == []
    # negative threshold + empty query: every node passes, each leaf is compared (similarity 0.0 > -1)
    l7 = leaves[7]
    empty = pkg.KmerMinHash(l7.num, l7.ksize, l7.is_protein, l7.seed, l7.max_hash, False)
    assert len(t.find(pkg.index.search_minhashes, empty, -1)) == 7
    assert t.find(pkg.index.search_minhashes_containment, empty, 0.0) == []
    # a node without min_n_below, reached in similarity mode
    js = json.load(open(path))
    del js["nodes"]["2"]["metadata"]["min_n_below"]
    json.dump(js, open(tmp_path / "v5.sbt.json", "w"))
    t2 = pkg.SBT.from_path(tmp_path / "v5.sbt.json")
    with pytest.raises(pkg.SourmashError):
        t2.find(pkg.index.search_minhashes, leaves[7], 0.0)
    assert [lf.pos for lf in t2.find(pkg.index.search_minhashes_containment, leaves[7], 0.5)] == \
        [lf.pos for lf in t.find(pkg.index.search_minhashes_containment, leaves[7], 0.5)]
    # an empty tree
    e = pkg.SBT.build([], [1009], ksize=1)
    assert e.find_many([leaves[7]], 0.0) == [[]] and len(e) == 0
