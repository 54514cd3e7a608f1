"""Collapsing a resident index by groups on the device (smh_index_collapse) against what a caller did before it: every sketch
read back to the host, np.unique over the concatenated members of each group, and a new index uploaded.

    python tools/bench_collapse.py [--sketches 10000] [--families 50] [--reps 3] [--threshold 0.03]
                                   [--out profiles/r19_bench_collapse.json]

The index is the pairwise index of tools/bench_search_many.py (`--sketches` splitmix64 sketches of about 5 000 hashes in
`--families` families).  The groupings:

  family     node i in group i mod families (G = families)
  cluster    the clusters of index.cluster(threshold, "jaccard") -- collapse(Clustering)
  identity   G = n, group = arange: the child equals the parent, so the floor is one device copy of the CSR (measured here
             with a torch clone of as many bytes)

and per grouping the union (min_fraction 0), the core (min_fraction 1) and the prevalence table (union with abund="count");
the identity runs the union alone.  The other route is index.sketches() + np.unique (return_counts) of the concatenated
members per group, the counts thresholded by need_g + ResidentIndex(...) of the new sketches.

Equal outputs (read() of both children) are asserted first.  Then the two routes are timed in turns, `reps` whole calls each
(the Python wrappers included), medians and the spread (max - min) reported.  The per-kernel timers come from a run of its own
under smh_profile_enable (HIP events).  The file is rewritten after every step: a run cut short leaves what it measured.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bench_gather as BG  # noqa: E402  (h(), sketch_of(), prof(); loads the package)
import bench_search_many as BS  # noqa: E402  (the pairwise index)

pkg = BG.pkg
TIMERS = ("collapse_count", "collapse_emit", "collapse_partition", "collapse_finish")


def profiled(fn):
    L = pkg.lib()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    fn()
    L.smh_profile_enable(0)
    out = {}
    for name in TIMERS:
        ms, k = BG.prof(name)
        out[name] = {"ms": ms, "entries": int(k)}
    return out


def host_route(index, group, n_groups, min_fraction, count):
    """the child index made on the host from the parent's sketches"""
    mins = [s.mins_np() for s in index.sketches()]
    first = index.nodes[0]
    members = [[] for _ in range(n_groups)]
    for v, g in enumerate(group):
        members[g].append(mins[v])
    made = []
    for part in members:
        mh = pkg.KmerMinHash(0, first.ksize, False, first.seed, first.max_hash, count)
        if part:
            hashes, c = np.unique(np.concatenate(part), return_counts=True)
            keep = c >= max(1, math.ceil(min_fraction * len(part)))
            if count:
                pkg.lib().smh_add_many_with_abund(mh._p, np.ascontiguousarray(hashes[keep]).ctypes.data_as(pkg.index.u64p),
                                                  np.ascontiguousarray(c[keep].astype(np.uint64)).ctypes.data_as(pkg.index.u64p), int(keep.sum()))
            else:
                mh.add_many(hashes[keep])
        made.append(mh)
    return pkg.index.ResidentIndex(made)


def same(a, b):
    x, y = a.read(), b.read()
    return all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(x, y))


def turns(mine, theirs, reps):
    a, b = [], []
    for _ in range(reps):     # in turns: other people's work shares the host
        t0 = time.perf_counter(); mine(); a.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); theirs(); b.append(time.perf_counter() - t0)
    return a, b


def spread(t):
    return {"s": t, "median_s": float(np.median(t)), "spread_s": float(max(t) - min(t))}


def copy_floor_ms(n_bytes, reps):
    """one device-to-device copy of n_bytes, HIP events through torch; None without torch"""
    try:
        import torch
    except ImportError:
        return None
    src = torch.empty(n_bytes // 8, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(src)
    dst.copy_(src)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); dst.copy_(src); b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def dump(out, path):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=10000)
    ap.add_argument("--families", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.03)
    ap.add_argument("--out", default=os.path.join("profiles", "r19_bench_collapse.json"))
    a = ap.parse_args()
    lane_max, wave_max, tile = pkg.matrix.collapse_geometry()
    n = a.sketches
    t0 = time.perf_counter()
    sketches = BS.make_family_sketches(n, a.families)
    index = pkg.index.ResidentIndex([BG.sketch_of(s) for s in sketches])
    total = int(index.sizes().sum())
    print("index %.1f s: %d sketches in %d families, %d resident hashes" % (time.perf_counter() - t0, n, a.families, total), flush=True)
    out = {"tool": "tools/bench_collapse.py", "sketches": n, "families": a.families, "resident_hashes": total, "reps": a.reps,
           "threshold": a.threshold, "geometry": {"lane_max": lane_max, "wave_max": wave_max, "group_tile": tile}, "runs": []}
    t0 = time.perf_counter()
    index.collapse([0] * n, 1)     # builds the hash directory, which the index keeps: not part of any timed call
    out["first_call_with_directory_s"] = time.perf_counter() - t0
    clustering = index.cluster(a.threshold, "jaccard")
    groupings = [("family", [i % a.families for i in range(n)], a.families),
                 ("cluster", clustering.cluster.tolist(), clustering.n_clusters),
                 ("identity", list(range(n)), n)]
    for name, group, G in groupings:
        modes = [("union", 0.0, "flat")] if name == "identity" else [("union", 0.0, "flat"), ("core", 1.0, "flat"), ("count", 0.0, "count")]
        for what, fraction, abund in modes:
            def dev():
                return index.collapse(group, G, 1, fraction, abund)

            def host():
                return host_route(index, group, G, fraction, abund == "count")

            child = dev()
            assert same(child, host()), "collapse and the host route differ: %s %s" % (name, what)
            t_dev, t_host = turns(dev, host, a.reps)
            run = {"grouping": name, "what": what, "groups": int(G), "child_hashes": int(child.sizes().sum()),
                   "collapse": spread(t_dev), "host_route": spread(t_host),
                   "ratio_host_over_collapse": float(np.median(t_host) / np.median(t_dev)), "timers": profiled(dev)}
            if name == "identity":
                run["copy_floor_ms"] = copy_floor_ms(8 * total, a.reps)
            del child
            print("%s %s: %s" % (name, what, json.dumps(run)), flush=True)
            out["runs"].append(run)
            dump(out, a.out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
