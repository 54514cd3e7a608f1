"""The nearest neighbours of a batch (smh_index_nearest_many) against what a caller did before it: search_many with
threshold 0 -- every pair that shares a hash -- then a numpy lexsort by (query, value descending, node) and a cut at k on the
host; and the k-nearest-neighbour graph (smh_index_nearest_self) against pairwise(threshold=0, upper=False) and the same host
sort.

    python tools/bench_nearest.py [--sketches 20000] [--qs 1,16,256] [--ks 1,10,100] [--knn 10000] [--families 50] [--knn-k 10]
                                  [--reps 3] [--out profiles/r22_bench_nearest.json]

The indexes and the queries are those of tools/bench_search_many.py (its 20 000-sketch index with nested batches of relatives;
its 10 000-sketch family index).  For every point the rows of both routes are asserted equal, integer for integer and in
order, before anything is timed.  Then both are timed in turns, `reps` runs each, whole call (the Python wrapper and the host
sort included); the kernel timers come from a separate run of each route under smh_profile_enable (HIP events).  The bytes each
route brings back to the host are recorded.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_gather as BG  # noqa: E402  (the index, h(), sketch_of(); loads the package)
import bench_search_many as BS  # noqa: E402  (make_query, make_family_sketches, dump)

pkg = BG.pkg
METRIC = "jaccard"
TIMERS = ("search_many_probe", "search_many_select", "search_many_emit", "nearest_clamp", "nearest_tile", "nearest_merge")


def timers():
    out = {}
    for name in TIMERS:
        ms, k = BG.prof(name)
        out[name] = {"ms": ms, "entries": int(k)}
    return out


def host_top_k(res, k):
    """(offsets, node, common, node_size, query_size) of the first k rows per query of a SearchResult ordered on the host"""
    q = res.query()
    order = np.lexsort((res.node, -getattr(res, METRIC), q))
    off = res.offsets.astype(np.int64)
    rank = np.arange(len(order), dtype=np.int64) - off[q[order]]        # (q[order] ascends: the rank inside the query)
    pick = order[rank < k]
    kept = np.minimum(np.diff(off), k)
    return np.concatenate([[0], np.cumsum(kept)]).astype(np.uint64), res.node[pick], res.common[pick], res.node_size[pick], res.query_size[pick]


def same(res, theirs):
    off, node, common, node_size, query_size = theirs
    return (np.array_equal(res.offsets, off) and np.array_equal(res.node, node) and np.array_equal(res.common, common)
            and np.array_equal(res.node_size, node_size) and np.array_equal(res.query_size, query_size))


def measure(mine, other, k, reps, what):
    """both routes: equality first, then `reps` runs each in turns, then one run each under the kernel timers"""
    L = pkg.lib()
    res, full = mine(), other()
    assert same(res, host_top_k(full, k)), "%s: the device's rows and the host-sorted rows differ" % what
    t_mine, t_other = [], []
    for _ in range(reps):     # in turns: other people's work shares the host
        t0 = time.perf_counter(); mine(); t_mine.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); host_top_k(other(), k); t_other.append(time.perf_counter() - t0)
    L.smh_profile_reset(); L.smh_profile_enable(1)
    mine()
    L.smh_profile_enable(0)
    t_dev = timers()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    other()
    L.smh_profile_enable(0)
    t_full = timers()
    m, o = float(np.median(t_mine)), float(np.median(t_other))
    nq = len(res.offsets) - 1
    return {"k": k, "rows": len(res), "rows_other_route": len(full), "nearest_s": t_mine, "nearest_median_s": m,
            "search_sort_s": t_other, "search_sort_median_s": o, "ratio_search_sort_over_nearest": o / m,
            "bytes_back_nearest": 16 * len(res) + 8 * (nq + 1), "bytes_back_search": 16 * len(full) + 8 * (nq + 1),
            "timers_nearest": t_dev, "timers_search": t_full}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=20000)
    ap.add_argument("--qs", default="1,16,256")
    ap.add_argument("--ks", default="1,10,100")
    ap.add_argument("--knn", type=int, default=10000)
    ap.add_argument("--families", type=int, default=50)
    ap.add_argument("--knn-k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r22_bench_nearest.json"))
    a = ap.parse_args()
    qs = sorted(int(x) for x in a.qs.split(",") if x)
    ks = sorted(int(x) for x in a.ks.split(",") if x)
    max_k, tile, slots = pkg.matrix.nearest_geometry()
    out = {"tool": "tools/bench_nearest.py", "metric": METRIC, "threshold": 0.0, "reps": a.reps, "budget": pkg.matrix.search_many_budget(),
           "geometry": {"max_k": max_k, "node_tile": tile, "merge_slots": slots}, "batches": [], "knn": None}

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
                hashes = BS.make_query(len(queries), sketches, every)
                queries.append(BG.sketch_of(hashes))      # a bulk fold: the query's state stays in HBM
                sizes.append(int(hashes.size))
            batch = queries[:Q]
            for k in ks:
                row = {"Q": Q, "query_hashes_total": int(sum(sizes[:Q]))}
                row.update(measure(lambda: index.nearest(batch, k, METRIC), lambda: index.search_many(batch, 0.0, METRIC), k, a.reps,
                                   "Q = %d, k = %d" % (Q, k)))
                out["batches"].append(row)
                print("Q = %d, k = %d: %s" % (Q, k, json.dumps(row)), flush=True)
                BS.dump(out, a.out)
        del index, queries, sketches, every

    if a.knn:
        n, k = a.knn, a.knn_k
        t0 = time.perf_counter()
        sketches = BS.make_family_sketches(n, a.families)
        index = pkg.index.ResidentIndex([BG.sketch_of(s) for s in sketches])
        total = int(sum(s.size for s in sketches))
        print("knn index %.1f s: %d sketches in %d families, %d resident hashes" % (time.perf_counter() - t0, n, a.families, total), flush=True)
        row = {"sketches": n, "families": a.families, "resident_hashes": total}
        row.update(measure(lambda: index.knn(k, METRIC), lambda: index.pairwise(0.0, METRIC, upper=False), k, a.reps, "knn(%d)" % k))
        out["knn"] = row
        print("knn: %s" % json.dumps(row), flush=True)
        BS.dump(out, a.out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
