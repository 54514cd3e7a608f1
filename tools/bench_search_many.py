"""The thresholded search of a batch (smh_index_search_many) against what a caller did before it: a loop over
ResidentIndex.find, one device call and one pass over the resident hashes per query; and the index against itself
(smh_index_search_self) against ResidentIndex.compare followed by thresholding the dense matrix on the host.

    python tools/bench_search_many.py [--sketches 20000] [--qs 1,16,64,256] [--pairwise 10000] [--families 50] [--reps 3]
                                      [--threshold 0.03] [--out profiles/r17_bench_search_many.json]

Batch: the index is that of tools/bench_gather.py (20 000 splitmix64 sketches of about 5 000 hashes in 200 families).  Query q
is sketch (q * 7919) mod n with the hashes dropped for which splitmix64(8_000_017 + q, j) >= 2^63 * 1.4 (about 30 %), plus
1 500 foreign hashes h(9_000_001 + q, j) that no sketch holds: a relative of one node and of its family.  The batches are
nested.  For every Q the node lists of search_many (jaccard) and of the loop over find are asserted equal before anything is
timed.  Then both are timed in turns, `reps` runs each, whole call (the Python wrapper included); the three timers come from a
separate search_many run under smh_profile_enable (HIP events).

Pairwise: `--pairwise` sketches of the same recipe in `--families` families.  pairwise(upper=True) against
compare(want=("jaccard",)) + numpy thresholding of the upper triangle; equal pairs asserted first; the bytes each route brings
back to the host are recorded.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_gather as BG  # noqa: E402  (the index, h(), sketch_of(); loads the package)

pkg = BG.pkg
splitmix64 = BG.splitmix64


def make_family_sketches(n, families):
    """BG.make_sketches with `families` pools instead of 200"""
    pools = [BG.h(5_000_011 + f, 2000) for f in range(families)]
    out = []
    for i in range(n):
        keep = splitmix64(7_000_003 + 2 * i + 1, np.arange(2000, dtype=np.uint64)) < np.uint64(1 << 63)
        out.append(np.unique(np.concatenate([BG.h(7_000_003 + 2 * i, 4000 + (37 * i) % 500), pools[i % families][keep]])))
    return out


def make_query(q, sketches, every):
    base = sketches[(q * 7919) % len(sketches)]
    keep = splitmix64(8_000_017 + q, np.arange(base.size, dtype=np.uint64)) < np.uint64(int((1 << 63) * 1.4))
    cand = np.unique(BG.h(9_000_001 + q, 1500))
    at = np.minimum(np.searchsorted(every, cand), every.size - 1)
    return np.union1d(base[keep], cand[every[at] != cand])


def timers():
    out = {}
    for name in ("search_many_probe", "search_many_select", "search_many_emit"):
        ms, k = BG.prof(name)
        out[name] = {"ms": ms, "entries": int(k)}
    return out


def dump(out, path):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as fh:     # after every step: a run cut short leaves what it measured
        json.dump(out, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=20000)
    ap.add_argument("--qs", default="1,16,64,256")
    ap.add_argument("--pairwise", type=int, default=10000)
    ap.add_argument("--families", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.03)
    ap.add_argument("--out", default=os.path.join("profiles", "r17_bench_search_many.json"))
    a = ap.parse_args()
    qs = sorted(int(x) for x in a.qs.split(",") if x)
    L = pkg.lib()
    short_owners, tile, max_queries = pkg.matrix.search_geometry()
    out = {"tool": "tools/bench_search_many.py", "metric": "jaccard", "threshold": a.threshold, "reps": a.reps,
           "budget": pkg.matrix.search_many_budget(), "geometry": {"short_owners": short_owners, "node_tile": tile, "max_queries": max_queries},
           "batches": [], "pairwise": None}

    if qs:
        t0 = time.perf_counter()
        sketches = BG.make_sketches(a.sketches)
        every = np.unique(np.concatenate(sketches))
        index = pkg.index.ResidentIndex([BG.sketch_of(s) for s in sketches])
        total = int(sum(s.size for s in sketches))
        out.update(sketches=a.sketches, resident_hashes=total)
        print("index %.1f s: %d sketches, %d resident hashes" % (time.perf_counter() - t0, a.sketches, total), flush=True)
        queries, sizes = [], []
        for Q in qs:
            while len(queries) < Q:
                hashes = make_query(len(queries), sketches, every)
                queries.append(BG.sketch_of(hashes))      # a bulk fold: the query's state stays in HBM
                sizes.append(int(hashes.size))
            batch = queries[:Q]

            def many():
                return index.search_many(batch, a.threshold, "jaccard")

            def loop():
                return [index.find(q, a.threshold) for q in batch]

            res, theirs = many(), loop()
            mine = [res.node[res.rows_of(q)].tolist() for q in range(Q)]
            assert mine == theirs, "search_many and the loop over find give different nodes (Q = %d)" % Q
            t_many, t_loop = [], []
            for _ in range(a.reps):     # in turns: other people's work shares the host
                t0 = time.perf_counter(); many(); t_many.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); loop(); t_loop.append(time.perf_counter() - t0)
            L.smh_profile_reset(); L.smh_profile_enable(1)
            many()
            L.smh_profile_enable(0)
            m, lo = float(np.median(t_many)), float(np.median(t_loop))
            row = {"Q": Q, "query_hashes_total": int(sum(sizes[:Q])), "rows": len(res),
                   "search_many_s": t_many, "search_many_median_s": m, "loop_s": t_loop, "loop_median_s": lo,
                   "ratio_loop_over_many": lo / m, "bytes_back_search_many": 16 * len(res) + 8 * (Q + 1),
                   "bytes_back_loop": 8 * a.sketches * Q, "timers": timers()}
            out["batches"].append(row)
            print("Q = %d: %s" % (Q, json.dumps(row)), flush=True)
            dump(out, a.out)
        del index, queries, sketches, every

    if a.pairwise:
        n = a.pairwise
        t0 = time.perf_counter()
        sketches = make_family_sketches(n, a.families)
        index = pkg.index.ResidentIndex([BG.sketch_of(s) for s in sketches])
        total = int(sum(s.size for s in sketches))
        print("pairwise index %.1f s: %d sketches in %d families, %d resident hashes" % (time.perf_counter() - t0, n, a.families, total),
              flush=True)

        def sparse():
            return index.pairwise(a.threshold, "jaccard", upper=True)

        def dense():
            J = index.compare(index, want=("jaccard",))["jaccard"]
            rows, cols = np.nonzero(np.triu(J > a.threshold, 1))
            return rows, cols

        res = sparse()
        rows, cols = dense()
        assert np.array_equal(res.query(), rows.astype(np.uint32)) and np.array_equal(res.node, cols.astype(np.uint32)), \
            "pairwise and compare + host threshold give different pairs"
        t_sparse, t_dense = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); sparse(); t_sparse.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); dense(); t_dense.append(time.perf_counter() - t0)
        L.smh_profile_reset(); L.smh_profile_enable(1)
        sparse()
        L.smh_profile_enable(0)
        m, d = float(np.median(t_sparse)), float(np.median(t_dense))
        out["pairwise"] = {"sketches": n, "families": a.families, "resident_hashes": total, "pairs": len(res),
                           "pairwise_s": t_sparse, "pairwise_median_s": m, "compare_threshold_s": t_dense, "compare_threshold_median_s": d,
                           "ratio_compare_over_pairwise": d / m, "bytes_back_pairwise": 16 * len(res) + 8 * (n + 1),
                           "bytes_back_compare": 8 * n * n, "timers": timers()}
        print("pairwise: %s" % json.dumps(out["pairwise"]), flush=True)
        dump(out, a.out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
