"""Writes the SBT fixtures of tests/golden/ from the reference's test data (run once, by hand, where the reference is
checked out: `python make_sbt_fixtures.py REFERENCE_ROOT`; no test reads the reference):

  sbt_v5/internal.0 .. internal.5   the .sbt.v5 nodegraphs, verbatim
  subset.sbt.json                   the 100-leaf layout of .sbt.subset (its leaf filenames key sbt_subset_sigs.json.gz)
  sbt_subset_nodes.json             per internal node of .sbt.subset: sha256 of its table bytes, per-table popcounts,
                                    min_n_below and the header's n_occupied (the 99 files are 4.9 MB)
  sbt_find_expected.json            the ordered results of SBT::find for every leaf of both trees as the query

Before writing, it checks what the tree build relies on: every internal nodegraph equals the bloom filter of the union
of the mins of the leaves below it, min_n_below is the smallest leaf size below, and n_occupied is the popcount of
table 0 (in the v5 files)."""
import gzip
import hashlib
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sbt_restatement as R  # noqa: E402

DATA = None   # the reference checkout's tests/data (first argument: the checkout's root)
THRESHOLDS = [0, 0.05, 0.1, 0.3, 0.5, 0.9, 1.0]


def leaf_sketch(storage, filename):
    return json.load(open(os.path.join(storage, filename)))[0]["signatures"][0]


def check_tree(json_name, check_occ):
    tree = json.load(open(os.path.join(DATA, json_name)))
    storage = os.path.join(DATA, tree["storage"]["args"]["path"])
    d = tree["d"]
    leaves = {int(p): sorted(leaf_sketch(storage, v["filename"])["mins"]) for p, v in tree["leaves"].items()}
    nums = {int(p): leaf_sketch(storage, v["filename"])["num"] for p, v in tree["leaves"].items()}
    maxh = {int(p): leaf_sketch(storage, v["filename"])["max_hash"] for p, v in tree["leaves"].items()}
    nodes, info = {}, {}
    sizes = None
    for p, v in tree["nodes"].items():
        raw = open(os.path.join(storage, v["filename"]), "rb").read()
        ksize, occ, sizes, tables = R.load_nodegraph(raw)
        nodes[int(p)] = (tables, v["metadata"].get("min_n_below"))
        info[int(p)] = dict(sha256=hashlib.sha256(R.table_bytes(tables)).hexdigest(),
                            popcounts=[int(t.sum()) for t in tables], min_n_below=v["metadata"]["min_n_below"],
                            n_occupied=occ)
        if check_occ:
            assert occ == int(tables[0].sum()), (json_name, p)
    built = R.build_nodes(d, leaves, sizes)
    assert set(built) == set(nodes)
    for p, (tables, mnb) in built.items():
        assert all((a == b).all() for a, b in zip(tables, nodes[p][0])), (json_name, p)
        assert mnb == nodes[p][1], (json_name, p)
    # num: the leaf sketch's own (0 for scaled sketches, src/lib.rs Q9)
    lv = {p: (leaves[p], nums[p] if maxh[p] == 0 else 0) for p in leaves}
    expected = []
    for qpos in sorted(leaves):
        for thr in THRESHOLDS:
            for cont in (False, True):
                hits = R.find(d, sizes, nodes, lv, leaves[qpos], thr, cont)
                expected.append(dict(query=qpos, threshold=thr, containment=cont, hits=hits))
    return tree, storage, info, expected


def main():
    global DATA
    DATA = os.path.join(sys.argv[1], "tests", "data")
    v5, v5_storage, _, v5_expected = check_tree("v5.sbt.json", True)
    sub, _, sub_info, sub_expected = check_tree("subset.sbt.json", False)
    out = os.path.join(HERE, "sbt_v5")
    for i in range(6):
        shutil.copyfile(os.path.join(v5_storage, "internal.%d" % i), os.path.join(out, "internal.%d" % i))
    for i in range(3):   # the reference's nodegraph unit tests read tests/data/internal.{0,1,2}: the same bytes
        assert open(os.path.join(DATA, "internal.%d" % i), "rb").read() == open(os.path.join(out, "internal.%d" % i), "rb").read()
    with open(os.path.join(HERE, "subset.sbt.json"), "w") as fh:
        json.dump(sub, fh, sort_keys=True)
    with gzip.open(os.path.join(HERE, "sbt_subset_sigs.json.gz"), "rt") as fh:
        assert set(json.load(fh)) == {v["filename"] for v in sub["leaves"].values()}
    with open(os.path.join(HERE, "sbt_subset_nodes.json"), "w") as fh:
        json.dump({str(k): sub_info[k] for k in sorted(sub_info)}, fh, sort_keys=True)
    with open(os.path.join(HERE, "sbt_find_expected.json"), "w") as fh:
        json.dump({"v5": v5_expected, "subset": sub_expected}, fh, separators=(",", ":"))


if __name__ == "__main__":
    main()
