"""Clustering on the device (smh_index_cluster) against what a caller did before it: ResidentIndex.pairwise, the rows brought
to the host, and a union-find or a greedy selection over them in Python.

    python tools/bench_cluster.py [--sketches 10000] [--families 50] [--reps 3] [--threshold 0.03]
                                  [--out profiles/r18_bench_cluster.json]

The index is the pairwise index of tools/bench_search_many.py (`--sketches` splitmix64 sketches of about 5 000 hashes in
`--families` families), the metric jaccard, the threshold that run's.  Per size:

  components   cluster(linkage="components") against pairwise(upper=True) + a union-find over its rows (plain Python, path
               halving, the larger root under the smaller) + numbering and representatives with numpy.
  greedy       cluster(linkage="greedy") against pairwise(upper=False) + the greedy of tests/cluster_restatement.py over
               adjacency dicts built from the rows.

Equal outputs are asserted first.  Then each pair of routes is timed in turns, `reps` whole calls each (the Python wrapper
included), medians reported.  The per-kernel timers come from runs of their own under smh_profile_enable (HIP events):
cluster_probe of the components run stands next to search_many_probe of a pairwise(upper=True) run on the same index.  The
bytes each route brings back to the host are recorded.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import bench_gather as BG  # noqa: E402  (h(), sketch_of(), prof(); loads the package)
import bench_search_many as BS  # noqa: E402  (the pairwise index)
import cluster_restatement as CR  # noqa: E402

pkg = BG.pkg
TIMERS = ("cluster_probe", "cluster_link", "cluster_finish", "cluster_round", "cluster_assign", "search_many_probe", "search_many_select",
          "search_many_emit")


def timers():
    out = {}
    for name in TIMERS:
        ms, k = BG.prof(name)
        if k:
            out[name] = {"ms": ms, "entries": int(k)}
    return out


def profiled(fn):
    L = pkg.lib()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    fn()
    L.smh_profile_enable(0)
    return timers()


def host_components(res, sizes):
    """(cluster, representative, n_clusters) from the rows of pairwise(upper=True)"""
    n = len(sizes)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for q, i in zip(res.query().tolist(), res.node.tolist()):
        a, b = find(q), find(i)
        if a != b:
            if a < b:
                parent[b] = a
            else:
                parent[a] = b
    root = np.array([find(v) for v in range(n)], dtype=np.int64)     # a root is its component's smallest node
    roots, cluster = np.unique(root, return_inverse=True)
    order = np.lexsort((np.arange(n), -sizes.astype(np.int64)))       # priority: size descending, node ascending
    rep_of_root = np.full(n, -1, dtype=np.int64)
    rep_of_root[root[order[::-1]]] = order[::-1]                      # the first in priority is written last
    return cluster.astype(np.uint32), rep_of_root[root].astype(np.uint32), len(roots)


def host_greedy(res, sizes):
    """the restatement's greedy over adjacency dicts built from the rows of pairwise(upper=False)"""
    n = len(sizes)
    adj = [dict() for _ in range(n)]
    for q, i, v, c in zip(res.query().tolist(), res.node.tolist(), res.jaccard.tolist(), res.common.tolist()):
        adj[q][i] = (v, c)
    sz = sizes.tolist()
    return CR.greedy(adj, sz, sz)


def turns(mine, theirs, reps):
    a, b = [], []
    for _ in range(reps):     # in turns: other people's work shares the host
        t0 = time.perf_counter(); mine(); a.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); theirs(); b.append(time.perf_counter() - t0)
    return a, b


def dump(out, path):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as fh:     # after every step: a run cut short leaves what it measured
        json.dump(out, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", default="10000")
    ap.add_argument("--families", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.03)
    ap.add_argument("--out", default=os.path.join("profiles", "r18_bench_cluster.json"))
    a = ap.parse_args()
    lane_max, tile = pkg.matrix.cluster_geometry()
    out = {"tool": "tools/bench_cluster.py", "metric": "jaccard", "threshold": a.threshold, "reps": a.reps, "families": a.families,
           "search_budget": pkg.matrix.search_many_budget(), "pair_budget": pkg.matrix.cluster_pair_budget(),
           "rounds_per_sync": pkg.matrix.cluster_rounds(), "geometry": {"lane_max": lane_max, "node_tile": tile}, "sizes": []}
    for n in (int(x) for x in a.sketches.split(",") if x):
        t0 = time.perf_counter()
        sketches = BS.make_family_sketches(n, a.families)
        index = pkg.index.ResidentIndex([BG.sketch_of(s) for s in sketches])
        sizes = index.sizes()
        total = int(sizes.sum())
        print("index %.1f s: %d sketches in %d families, %d resident hashes" % (time.perf_counter() - t0, n, a.families, total), flush=True)
        row = {"sketches": n, "resident_hashes": total}

        # ---- components
        def dev_components():
            return index.cluster(a.threshold, "jaccard", "components")

        def upper():
            return index.pairwise(a.threshold, "jaccard", upper=True)

        def host_route_components():
            return host_components(upper(), sizes)

        got, (cl, rep, k) = dev_components(), host_route_components()
        assert np.array_equal(got.cluster, cl) and np.array_equal(got.representative, rep) and got.n_clusters == k, \
            "cluster(components) and pairwise + host union-find differ"
        pairs = len(upper())
        t_dev, t_host = turns(dev_components, host_route_components, a.reps)
        t_rows, _ = turns(upper, lambda: None, a.reps)
        row["components"] = {
            "clusters": int(k), "largest": int(got.sizes().max()), "pairs_upper": pairs,
            "cluster_s": t_dev, "cluster_median_s": float(np.median(t_dev)),
            "pairwise_union_find_s": t_host, "pairwise_union_find_median_s": float(np.median(t_host)),
            "pairwise_alone_s": t_rows, "pairwise_alone_median_s": float(np.median(t_rows)),
            "ratio_host_over_cluster": float(np.median(t_host) / np.median(t_dev)),
            "ratio_pairwise_alone_over_cluster": float(np.median(t_rows) / np.median(t_dev)),
            "bytes_back_cluster": 8 * n + 4, "bytes_back_pairwise": 16 * pairs + 8 * (n + 1),
            "timers_cluster": profiled(dev_components), "timers_pairwise_upper": profiled(upper)}
        print("components: %s" % json.dumps(row["components"]), flush=True)
        out["sizes"].append(row)
        dump(out, a.out)

        # ---- greedy
        def dev_greedy():
            return index.cluster(a.threshold, "jaccard", "greedy")

        def full():
            return index.pairwise(a.threshold, "jaccard", upper=False)

        def host_route_greedy():
            return host_greedy(full(), sizes)

        got, (cl, rep, common, k) = dev_greedy(), host_route_greedy()
        assert got.cluster.tolist() == cl and got.representative.tolist() == rep and got.rep_common.tolist() == common and \
            got.n_clusters == k, "cluster(greedy) and pairwise + the restatement's greedy differ"
        sz = sizes.tolist()
        adj = [dict() for _ in range(n)]
        res = full()
        for q, i in zip(res.query().tolist(), res.node.tolist()):
            adj[q][i] = (0.0, 0)
        rounds = CR.greedy_rounds(adj, sz)[1]
        directed = len(res)
        del adj, res
        t_dev, t_host = turns(dev_greedy, host_route_greedy, a.reps)
        row["greedy"] = {
            "clusters": int(k), "largest": int(got.sizes().max()), "pairs_directed": directed, "rounds": rounds,
            "cluster_s": t_dev, "cluster_median_s": float(np.median(t_dev)),
            "pairwise_greedy_s": t_host, "pairwise_greedy_median_s": float(np.median(t_host)),
            "ratio_host_over_cluster": float(np.median(t_host) / np.median(t_dev)),
            "bytes_back_cluster": 12 * n + 4, "bytes_back_pairwise": 16 * directed + 8 * (n + 1),
            "adjacency_bytes_device": 8 * directed, "timers_cluster": profiled(dev_greedy)}
        print("greedy: %s" % json.dumps(row["greedy"]), flush=True)
        dump(out, a.out)
        del index, sketches
    print(json.dumps(out))


if __name__ == "__main__":
    main()
