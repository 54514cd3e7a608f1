"""Gather (smh_index_gather) against the only thing a caller could do before it: a host loop over
ResidentIndex.most_common that rebuilds and re-uploads the remaining query every round.

    python tools/bench_gather.py [--sketches 20000] [--picked 500] [--reps 3] [--loop-reps 2] [--out profiles/r10_bench_gather.json]

Input (deterministic; h(seed, j) = splitmix64(seed, j) >> 10, which lies below max_hash = 2^64 // 1000, scaled = 1000):
    family pool f (200 families)   h(5_000_011 + f, j)          for j < 2000
    sketch i                       h(7_000_003 + 2 i, j)        for j < 4000 + (37 i mod 500)          (private)
                                 + pool (i mod 200) entries j with splitmix64(7_000_003 + 2 i + 1, j) < 2^63   (about 1000)
    query                          the union of the sketches i with i mod (sketches / picked) == 7  (`picked` of them)
                                 + as many hashes again, h(9_000_001, j) for j < that number, which belong to no sketch
The two decompositions (match, common_remaining per round) are asserted equal before anything is timed.  Then gather and
the loop are timed in turns; the kernels' share comes from a separate gather run under smh_profile_enable (HIP events).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (maps torch's HIP runtime first)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
from sourmash_rust_amd.synth import splitmix64  # noqa: E402

SCALED = 1000
MAX_HASH = (1 << 64) // SCALED


def h(seed, n):
    return splitmix64(seed, np.arange(n, dtype=np.uint64)) >> np.uint64(10)


def make_sketches(n):
    pools = [h(5_000_011 + f, 2000) for f in range(200)]
    out = []
    for i in range(n):
        keep = splitmix64(7_000_003 + 2 * i + 1, np.arange(2000, dtype=np.uint64)) < np.uint64(1 << 63)
        out.append(np.unique(np.concatenate([h(7_000_003 + 2 * i, 4000 + (37 * i) % 500), pools[i % 200][keep]])))
    return out


def sketch_of(hashes):
    mh = pkg.KmerMinHash(0, 31, False, 42, MAX_HASH, False)
    mh.add_many(hashes)
    return mh


def host_loop(index, sketches, query, threshold):
    """what a caller could do without gather: arg-max on the device, removal and re-upload on the host"""
    remaining = query
    rows = []
    while remaining.size:
        pos, common = index.most_common(sketch_of(remaining))
        if common < threshold:
            break
        rows.append((pos, common))
        remaining = remaining[~np.isin(remaining, sketches[pos], assume_unique=True)]
    return rows


def prof(name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return ms.value, k.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=20000)
    ap.add_argument("--picked", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-reps", type=int, default=2)
    ap.add_argument("--threshold", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "r10_bench_gather.json"))
    a = ap.parse_args()

    t0 = time.perf_counter()
    sketches = make_sketches(a.sketches)
    step = a.sketches // a.picked
    picked = [i for i in range(a.sketches) if i % step == 7 % step][:a.picked]
    inside = np.unique(np.concatenate([sketches[i] for i in picked]))
    every = np.unique(np.concatenate(sketches))
    outside = np.setdiff1d(np.unique(h(9_000_001, inside.size)), every, assume_unique=True)
    query_hashes = np.union1d(inside, outside)
    del every
    nodes = [sketch_of(s) for s in sketches]
    index = pkg.index.ResidentIndex(nodes)
    query = sketch_of(query_hashes)          # a bulk fold: the query's state stays in HBM
    t_setup = time.perf_counter() - t0
    total = int(sum(s.size for s in sketches))
    print("setup %.1f s: %d sketches, %d resident hashes, query of %d hashes (%d from %d sketches)"
          % (t_setup, a.sketches, total, query_hashes.size, inside.size, len(picked)), flush=True)

    def gather():
        return index.gather(query, threshold_bp=a.threshold, scaled=1, abund_stats=False)

    res = gather()
    mine = [(r.match, r.common_remaining) for r in res.rows]
    t0 = time.perf_counter()
    theirs = host_loop(index, sketches, query_hashes, a.threshold)
    t_loop_first = time.perf_counter() - t0
    assert mine == theirs, "gather and the most_common loop decompose the query differently"
    print("equal decompositions: %d rounds (first loop run %.2f s)" % (len(mine), t_loop_first), flush=True)

    t_gather, t_loop = [], []
    for k in range(max(a.reps, a.loop_reps)):     # in turns: other people's work shares the host
        if k < a.reps:
            t0 = time.perf_counter(); gather(); t_gather.append(time.perf_counter() - t0)
        if k < a.loop_reps:
            t0 = time.perf_counter(); host_loop(index, sketches, query_hashes, a.threshold); t_loop.append(time.perf_counter() - t0)

    L = pkg.lib()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    gather()
    L.smh_profile_enable(0)
    hits_ms, _ = prof("gather_hits")
    inv_ms, _ = prof("gather_invert")
    rounds_ms, batches = prof("gather_rounds")
    n_rounds = len(mine)
    g, lo = float(np.median(t_gather)), float(np.median(t_loop))
    out = {
        "tool": "tools/bench_gather.py", "sketches": a.sketches, "resident_hashes": total, "query_hashes": int(query_hashes.size),
        "picked": len(picked), "threshold_common": a.threshold, "rounds": n_rounds,
        "rounds_per_sync": int(L.smh_gather_rounds_per_sync()),
        "gather_call_s": t_gather, "gather_call_median_s": g,
        "host_loop_s": t_loop, "host_loop_median_s": lo, "host_loop_first_run_s": t_loop_first,
        "ratio_loop_over_gather": lo / g,
        "kernel_ms": {"gather_hits": hits_ms, "gather_invert": inv_ms, "gather_rounds_total": rounds_ms,
                      "round_batches": int(batches), "per_round_us": 1e3 * rounds_ms / max(n_rounds, 1),
                      "prepare_ms": hits_ms + inv_ms},
    }
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
