"""Nodegraph on the host (reference src/index/nodegraph.rs:236-330), its file format and quirks, the SBT v5 layout, and
the tests' restatement of SBT::find against the recorded results.  No GPU needed."""
import gzip
import json
import os
import random

import pytest

from conftest import GOLDEN, sorted_sketch
import sbt_restatement as R

V5_SIZES = [99991, 99989, 99971, 99961]


def fixture(name):
    return open(os.path.join(GOLDEN, "sbt_v5", name), "rb").read()


def test_count_and_get(pkg):
    ng = pkg.Nodegraph([10], 3)
    assert ng.count(801084876663808)
    assert ng.get(801084876663808) == 1
    assert ng.unique_kmers() == 1 and ng.n_occupied_bins() == 1
    rng = random.Random(5)
    for _ in range(200):
        h = rng.getrandbits(64)
        g = pkg.Nodegraph([10], 3)
        g.count(h)
        assert g.get(h) == 1


@pytest.mark.parametrize("i", range(6))
def test_load_save_nodegraph(pkg, i):
    data = fixture("internal.%d" % i)
    ng = pkg.Nodegraph.from_buffer(data)
    assert ng.to_bytes() == data
    assert ng.unique_kmers() == 0
    assert ng.n_occupied_bins() == int.from_bytes(data[11:19], "little")


def test_update_nodegraph(pkg):
    parent = pkg.Nodegraph.from_buffer(fixture("internal.0"))
    ng = pkg.Nodegraph(V5_SIZES, 1)
    ng.update(pkg.Nodegraph.from_buffer(fixture("internal.1")))
    ng.update(pkg.Nodegraph.from_buffer(fixture("internal.2")))
    # the tables equal the parent's; update leaves the counters alone (nodegraph.rs:85-88)
    assert ng.to_bytes()[19:] == parent.to_bytes()[19:]
    assert ng.n_occupied_bins() == 0 and ng.unique_kmers() == 0


def test_load_nodegraph(pkg, tmp_path):
    p = tmp_path / "internal.0"
    p.write_bytes(fixture("internal.0"))
    ng = pkg.Nodegraph.from_path(p)
    assert ng.tablesizes() == V5_SIZES
    assert ng.get(1877811740) == 0
    for h in (1877811749, 1339603207230, 5641354835174, 10502027926594, 11550845136154, 801084876663808,
              802340523858506, 803596407436267):
        assert ng.get(h) == 1


def test_counters_similarity_containment(pkg):
    a, b = pkg.Nodegraph([101, 103], 5), pkg.Nodegraph([101, 103], 5)
    assert a.count(7) and not a.count(7)
    assert not a.count(7 + 101 * 103)   # a multiple of both sizes apart: the same bins
    assert a.count(7 + 101)             # same bin in table 0, a new one in table 1
    assert a.n_occupied_bins() == 3 and a.unique_kmers() == 2
    a2 = pkg.Nodegraph([101, 103], 5)
    for h in (1, 2, 3):
        a2.count(h)
    b.count(2); b.count(3); b.count(500)
    # intersection: bins of 2 and 3 in both tables (4 bits); union 2 x 4 bits
    bits_a = {(0, h % 101) for h in (1, 2, 3)} | {(1, h % 103) for h in (1, 2, 3)}
    bits_b = {(0, h % 101) for h in (2, 3, 500)} | {(1, h % 103) for h in (2, 3, 500)}
    assert a2.similarity(b) == len(bits_a & bits_b) / len(bits_a | bits_b)
    assert a2.containment(b) == len(bits_a & bits_b) / (101 + 103)


def test_size_multiple_of_8_is_written_one_byte_short(pkg):
    # nodegraph.rs:107-125 writes the last partial u32 block as ceil(rem / 8) bytes, while from_reader reads
    # size / 8 + 1 bytes per table: a size that is a multiple of 8 comes out one byte shorter than it is read back
    ng = pkg.Nodegraph([16], 1)
    ng.count(3)
    data = ng.to_bytes()
    assert len(data) == 19 + 8 + 2
    with pytest.raises(pkg.SourmashError):
        pkg.Nodegraph.from_buffer(data)
    # a two-table graph: the short first table makes the reader run one byte into the next table's header
    g2 = pkg.Nodegraph([64, 11], 1)
    assert len(g2.to_bytes()) == 19 + (8 + 8) + (8 + 2)
    odd = pkg.Nodegraph([17], 1)
    odd.count(16)
    assert len(odd.to_bytes()) == 19 + 8 + 3
    assert pkg.Nodegraph.from_buffer(odd.to_bytes()).to_bytes() == odd.to_bytes()


def test_bad_header_is_an_error(pkg):
    good = fixture("internal.1")
    for bad in (b"OXLX" + good[4:], good[:4] + b"\x05" + good[5:], good[:5] + b"\x01" + good[6:], good[:1000], b""):
        with pytest.raises(pkg.SourmashError):
            pkg.Nodegraph.from_buffer(bad)
    with pytest.raises(pkg.SourmashError):
        pkg.Nodegraph([0], 1)
    with pytest.raises(pkg.SourmashError):
        pkg.Nodegraph([1 << 32], 1)


def test_v5_layout():
    # sbt.rs:533-537
    tree = json.load(open(os.path.join(GOLDEN, "v5.sbt.json")))
    assert tree["d"] == 2 and tree["factory"]["args"] == [1, 100000, 4]
    assert len(tree["nodes"]) == 6 and len(tree["leaves"]) == 7
    for v in tree["nodes"].values():
        assert os.path.exists(os.path.join(GOLDEN, "sbt_v5", v["filename"]))


def v5_tree():
    tree = json.load(open(os.path.join(GOLDEN, "v5.sbt.json")))
    nodes, sizes = {}, None
    for p, v in tree["nodes"].items():
        _, _, sizes, tables = R.load_nodegraph(fixture(v["filename"]))
        nodes[int(p)] = (tables, v["metadata"]["min_n_below"])
    leaves = {}
    for p, v in tree["leaves"].items():
        sk = json.load(open(os.path.join(GOLDEN, "sbt_v5", v["filename"] + ".sig")))[0]["signatures"][0]
        leaves[int(p)] = (sorted(sk["mins"]), sk["num"])
    return tree["d"], sizes, nodes, leaves


def test_restatement_matches_recorded_results_v5():
    expected = json.load(open(os.path.join(GOLDEN, "sbt_find_expected.json")))["v5"]
    d, sizes, nodes, leaves = v5_tree()
    assert len(expected) == 7 * 7 * 2
    for e in expected:
        got = R.find(d, sizes, nodes, leaves, leaves[e["query"]][0], e["threshold"], e["containment"])
        assert got == e["hits"], e


def test_restatement_matches_recorded_results_subset():
    # the subset's node files are not committed: the restatement builds them from the leaves (the fixture generator
    # checked that this gives the reference's files, and sbt_subset_nodes.json records their digests)
    import hashlib
    expected = json.load(open(os.path.join(GOLDEN, "sbt_find_expected.json")))["subset"]
    tree = json.load(open(os.path.join(GOLDEN, "subset.sbt.json")))
    with gzip.open(os.path.join(GOLDEN, "sbt_subset_sigs.json.gz"), "rt") as fh:
        sigs = json.load(fh)
    leaves = {}
    for p, v in tree["leaves"].items():
        sk = sorted_sketch(sigs[v["filename"]][0]["signatures"][0])
        leaves[int(p)] = (sk["mins"], 0 if sk["max_hash"] else sk["num"])
    built = R.build_nodes(tree["d"], {p: m for p, (m, _) in leaves.items()}, V5_SIZES)
    recorded = json.load(open(os.path.join(GOLDEN, "sbt_subset_nodes.json")))
    assert set(map(int, recorded)) == set(built)
    for p, (tables, mnb) in built.items():
        r = recorded[str(p)]
        assert hashlib.sha256(R.table_bytes(tables)).hexdigest() == r["sha256"]
        assert mnb == r["min_n_below"]
    sample = set(sorted(leaves)[::9])
    for e in expected:
        if e["query"] in sample:
            got = R.find(tree["d"], V5_SIZES, built, leaves, leaves[e["query"]][0], e["threshold"], e["containment"])
            assert got == e["hits"], e
