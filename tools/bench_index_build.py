"""Building a resident index from records on the device (smh_index_from_sequences_dev) and concatenating indexes
(smh_index_concat) against the route that existed before: the grouped fold into one fresh host sketch per node
(smh_add_sequences_grouped_dev, what add_records_grouped runs) and ResidentIndex(sketches), which uploads them again.

    python tools/bench_index_build.py [--genomes 1000] [--genome-bp 5000000] [--reads 2000000] [--host-reads 20000]
                                      [--parts 10] [--part-nodes 1000] [--reps 3] [--out profiles/r20_bench_index_build.json]

Input (deterministic): consecutive pieces of the synthetic DNA stream of smh_synth_dna_dev (seed 7) in device memory;
k = 31, scaled = 1000, no abundances.  Shapes:

  genomes    `genomes` records of `genome-bp` bases, one node per genome
  reads      the first `host-reads` and the first `reads` records of 150 bases, one node per read (groups = NULL); the host
             route runs at `host-reads` only
  concat     `parts` indexes of `part-nodes` nodes (splitmix64 sketches of about 5 000 hashes) concatenated, against
             ResidentIndex(all nodes)

Equal read()s are asserted first.  Then the two routes are timed in turns, `reps` whole calls each (the Python wrappers
included), medians and the spread reported; the bytes that come back to the host are those of the offsets (8 (G + 1)) against
the hashes the host route reads and uploads.  The per-kernel timers come from a run of its own under smh_profile_enable.  The
file is rewritten after every step: a run cut short leaves what it measured.  No figure is claimed in advance.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (maps torch's HIP runtime first)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
from sourmash_rust_amd.errors import call  # noqa: E402
from sourmash_rust_amd.index import u32p, u64p  # noqa: E402
from sourmash_rust_amd.synth import splitmix64  # noqa: E402

KSIZE, MAX_HASH = 31, (1 << 64) // 1000
TIMERS = ("dna_rolling", "index_build_heads", "index_build_emit", "index_build_merge")
COUNTERS = ("index_build_fold", "index_built", "index_concat")


def prof(name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return ms.value, k.value


def profiled(fn):
    L = pkg.lib()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    fn()
    L.smh_profile_enable(0)
    return {name: dict(zip(("ms", "entries"), prof(name))) for name in TIMERS + COUNTERS}


def stream_tensor(start, length):
    t = torch.empty(length + 64, dtype=torch.uint8, device="cuda")
    call(pkg.lib().smh_synth_dna_dev, C.c_void_p(t.data_ptr()), start, length, 7, 0, None)
    torch.cuda.synchronize()
    return t


def fresh():
    return pkg.KmerMinHash(0, KSIZE, False, 42, MAX_HASH, False)


def host_route(t, offsets, n):
    """one fresh sketch per record through the grouped fold, then the upload"""
    sk = [fresh() for _ in range(n)]
    arr = (C.c_void_p * n)(*[m._p for m in sk])
    grp = np.arange(n, dtype=np.uint32)
    call(pkg.lib().smh_add_sequences_grouped_dev, arr, n, C.c_void_p(t.data_ptr()), int(offsets[-1]), offsets.ctypes.data_as(u64p),
         grp.ctypes.data_as(u32p), n, True, None)
    return pkg.index.ResidentIndex(sk)


def same(a, b):
    x, y = a.read(), b.read()
    return all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(x, y))


def turns(mine, theirs, reps):
    a, b = [], []
    for _ in range(reps):     # in turns: other people's work shares the host
        t0 = time.perf_counter(); mine(); a.append(time.perf_counter() - t0)
        if theirs is not None:
            t0 = time.perf_counter(); theirs(); b.append(time.perf_counter() - t0)
    return a, b


def spread(t):
    return {"s": t, "median_s": float(np.median(t)), "spread_s": float(max(t) - min(t))} if t else None


def dump(out, path):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


def build_shape(name, t, offsets, reps, with_host, out, path):
    n = len(offsets) - 1
    like = fresh()

    def dev():
        return pkg.index.ResidentIndex.from_records((t.data_ptr(), int(offsets[-1]), offsets), like)

    host = (lambda: host_route(t, offsets, n)) if with_host else None
    built = dev()
    hashes = int(built.sizes().sum())
    if with_host:
        assert same(built, host()), "the built index and the host route differ: %s" % name
    del built
    t_dev, t_host = turns(dev, host, reps)
    run = {"shape": name, "nodes": n, "bases": int(offsets[-1]), "hashes": hashes, "from_records": spread(t_dev), "host_route": spread(t_host),
           "bytes_back_from_records": 8 * (n + 1), "bytes_back_and_up_host_route": 16 * hashes if with_host else None,
           "ratio_host_over_from_records": float(np.median(t_host) / np.median(t_dev)) if with_host else None, "timers": profiled(dev)}
    print("%s: %s" % (name, json.dumps(run)), flush=True)
    out["runs"].append(run)
    dump(out, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=1000)
    ap.add_argument("--genome-bp", type=int, default=5000000)
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--host-reads", type=int, default=20000)
    ap.add_argument("--parts", type=int, default=10)
    ap.add_argument("--part-nodes", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r20_bench_index_build.json"))
    a = ap.parse_args()
    tile, threads = C.c_uint32(), C.c_uint32()
    pkg.lib().smh_index_build_geometry(C.byref(tile), C.byref(threads))
    out = {"tool": "tools/bench_index_build.py", "ksize": KSIZE, "scaled": 1000, "reps": a.reps, "budget": int(pkg.lib().smh_index_build_budget()),
           "geometry": {"tile_elems": tile.value, "threads": threads.value}, "runs": []}

    if a.genomes:
        t = stream_tensor(0, a.genomes * a.genome_bp)
        offsets = np.arange(a.genomes + 1, dtype=np.uint64) * np.uint64(a.genome_bp)
        build_shape("genomes", t, offsets, a.reps, True, out, a.out)
        del t
    if a.reads:
        t = stream_tensor(0, a.reads * 150)
        for n, with_host in ((min(a.host_reads, a.reads), True), (a.reads, False)):
            offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(150)
            build_shape("reads_%d" % n, t, offsets, a.reps, with_host, out, a.out)
        del t
    if a.parts:
        nodes = []
        for i in range(a.parts * a.part_nodes):
            mh = fresh()
            mh.add_many(np.unique(splitmix64(21_000_003 + i, np.arange(5000, dtype=np.uint64)) >> np.uint64(10)))
            nodes.append(mh)
        parts = [pkg.index.ResidentIndex(nodes[p * a.part_nodes:(p + 1) * a.part_nodes]) for p in range(a.parts)]

        def dev():
            return pkg.index.ResidentIndex.concat(parts)

        def host():
            return pkg.index.ResidentIndex(nodes)

        joined = dev()
        assert same(joined, host()), "concat and the index of all nodes differ"
        hashes = int(joined.sizes().sum())
        del joined
        t_dev, t_host = turns(dev, host, a.reps)
        run = {"shape": "concat", "parts": a.parts, "nodes": len(nodes), "hashes": hashes, "concat": spread(t_dev), "index_of_all_nodes": spread(t_host),
               "ratio_host_over_concat": float(np.median(t_host) / np.median(t_dev)), "timers": profiled(dev)}
        print("concat: %s" % json.dumps(run), flush=True)
        out["runs"].append(run)
        dump(out, a.out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
