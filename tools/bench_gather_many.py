"""Gather of a batch of queries (smh_index_gather_many) against what a caller did before it: a loop over
ResidentIndex.gather, one device call per query.

    python tools/bench_gather_many.py [--sketches 20000] [--qs 1,16,64,256,1024] [--reps 3] [--out profiles/r15_bench_gather_many.json]

The index is that of tools/bench_gather.py (20 000 splitmix64 sketches of about 5 000 hashes in 200 families).  Query q is
the union of a different random 50 .. 500 of the sketches (numpy default_rng(1000 + q)) plus as many foreign hashes,
h(9_000_001 + q, j), that no sketch holds.  The batches are nested: the batch of Q queries is the first Q of the largest.
For every Q the rows of gather_many and of the loop are asserted equal before anything is timed.  Then both are timed in
turns, `reps` runs each, whole call (the Python wrapper included, abund_stats=False); the three timers come from a separate
gather_many run under smh_profile_enable (HIP events).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_gather as BG  # noqa: E402  (the index, h(), sketch_of(); loads the package)

pkg = BG.pkg


def make_query(q, sketches, every):
    rng = np.random.default_rng(1000 + q)
    picked = rng.choice(len(sketches), int(rng.integers(50, 501)), replace=False)
    inside = np.unique(np.concatenate([sketches[i] for i in picked]))
    cand = np.unique(BG.h(9_000_001 + q, inside.size))
    at = np.minimum(np.searchsorted(every, cand), every.size - 1)
    return np.union1d(inside, cand[every[at] != cand]), len(picked)


def rows_of(results):
    return [[(r.match, r.common_remaining, r.common_original, r.size_match, r.abund_sum) for r in res.rows] for res in results]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=20000)
    ap.add_argument("--qs", default="1,16,64,256,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "r15_bench_gather_many.json"))
    a = ap.parse_args()
    qs = sorted(int(x) for x in a.qs.split(","))

    t0 = time.perf_counter()
    sketches = BG.make_sketches(a.sketches)
    every = np.unique(np.concatenate(sketches))
    index = pkg.index.ResidentIndex([BG.sketch_of(s) for s in sketches])
    total = int(sum(s.size for s in sketches))
    print("index %.1f s: %d sketches, %d resident hashes" % (time.perf_counter() - t0, a.sketches, total), flush=True)

    L = pkg.lib()
    kw = dict(threshold_bp=a.threshold, scaled=1, abund_stats=False)
    queries, picked, sizes = [], [], []
    out = {"tool": "tools/bench_gather_many.py", "sketches": a.sketches, "resident_hashes": total, "threshold_common": a.threshold,
           "rounds_per_sync": int(L.smh_gather_rounds_per_sync()), "budget": int(L.smh_gather_many_budget()), "reps": a.reps, "batches": []}
    for Q in qs:
        t0 = time.perf_counter()
        while len(queries) < Q:
            hashes, k = make_query(len(queries), sketches, every)
            queries.append(BG.sketch_of(hashes))      # a bulk fold: the query's state stays in HBM
            picked.append(k); sizes.append(int(hashes.size))
        batch = queries[:Q]
        t_setup = time.perf_counter() - t0

        def many():
            return index.gather_many(batch, **kw)

        def loop():
            return [index.gather(q, **kw) for q in batch]

        mine, theirs = rows_of(many()), rows_of(loop())
        assert mine == theirs, "gather_many and the loop over gather give different rows (Q = %d)" % Q
        rounds = [len(r) for r in mine]
        t_many, t_loop = [], []
        for _ in range(a.reps):     # in turns: other people's work shares the host
            t0 = time.perf_counter(); many(); t_many.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); loop(); t_loop.append(time.perf_counter() - t0)
        L.smh_profile_reset(); L.smh_profile_enable(1)
        many()
        L.smh_profile_enable(0)
        timers = {}
        for name in ("gather_many_probe", "gather_many_fill", "gather_many_rounds"):
            ms, k = BG.prof(name)
            timers[name] = {"ms": ms, "entries": int(k)}
        m, lo = float(np.median(t_many)), float(np.median(t_loop))
        row = {"Q": Q, "query_hashes_total": int(sum(sizes[:Q])), "sketches_picked_total": int(sum(picked[:Q])),
               "rounds_total": int(sum(rounds)), "rounds_longest": int(max(rounds)),
               "gather_many_s": t_many, "gather_many_median_s": m, "loop_s": t_loop, "loop_median_s": lo,
               "loop_spread_s": max(t_loop) - min(t_loop), "ratio_loop_over_many": lo / m, "timers": timers}
        out["batches"].append(row)
        print("Q = %d (queries made in %.1f s): %s" % (Q, t_setup, json.dumps(row)), flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:     # after every batch: a run cut short leaves what it measured
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
