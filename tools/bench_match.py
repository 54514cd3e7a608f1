"""Matching records against a resident index (smh_index_match_sequences_dev) next to two yardsticks: sketching the same
bytes into ONE scaled sketch (the floor: the hash kernel is shared and nothing is looked up), and the detour a caller had
before -- a sketch per record, all of them read back, a second index, an N x M compare, arg-max on the host -- at a size
where the detour still fits.

    python tools/bench_match.py [--reads 60000000] [--read-len 150] [--contigs 2000] [--contig-len 5000000]
                                [--sketches 10000] [--hashes 5000] [--planted 200] [--detour-reads 20000] [--reps 3]
                                [--out profiles/r14_bench_match.json]

Input (deterministic): the records are consecutive pieces of the synthetic DNA stream of smh_synth_dna_dev (seed 7), made
in device memory; k = 31, scaled = 1000.  Index node i holds the distinct values of splitmix64(14_000_003 + i, j) >> 10 for
j < hashes (below max_hash = 2^64 // 1000); the first `planted` nodes also hold the scaled sketch of 1 Mbp of the stream each
(node i: the stream from i Mbp on), so records cut from the first `planted` Mbp have a node to belong to.  The detour and
the match are asserted to agree on best_common before anything is timed.  Wall clock around calls that return with their
device work complete; the kernels' share from a separate run under smh_profile_enable.  No ratio is claimed in advance: the
figures are what the file says.
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
from sourmash_rust_amd.synth import splitmix64  # noqa: E402

KSIZE, MAX_HASH, MBP = 31, (1 << 64) // 1000, 1000000


def prof(name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return ms.value, k.value


def stream_tensor(start, length):
    t = torch.empty(length + 64, dtype=torch.uint8, device="cuda")
    call(pkg.lib().smh_synth_dna_dev, C.c_void_p(t.data_ptr()), start, length, 7, 0, None)
    return t


def fresh():
    return pkg.KmerMinHash(0, KSIZE, False, 42, MAX_HASH, False)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); out.append(time.perf_counter() - t0)
    return out


def shape(index, name, n_records, record_len, reps, detour_records):
    """one batch shape: match, the one-sketch floor, and the detour on its first `detour_records` records"""
    total = n_records * record_len
    seq = stream_tensor(0, total)
    off = np.arange(n_records + 1, dtype=np.uint64) * np.uint64(record_len)

    def match(n=n_records):
        return index.match((seq.data_ptr(), n * record_len, off[:n + 1]))

    def floor():
        fresh().add_sequences_dev(seq.data_ptr(), total, off, True)

    nd = min(detour_records, n_records)

    def detour():
        per = [fresh() for _ in range(nd)]
        flat = seq[:nd * record_len].cpu().numpy().tobytes()
        pkg.KmerMinHash.add_sequences_grouped(per, [flat[i * record_len:(i + 1) * record_len] for i in range(nd)], list(range(nd)), True)
        for m in per:
            m.mins_np()      # "read all those signatures back to the host"
        cc = pkg.index.ResidentIndex(per).compare(index, want=("count_common",))["count_common"]
        return cc.max(axis=1), cc.argmax(axis=1)

    res = match(nd)
    best_common, best = detour()
    assert np.array_equal(res.best_common, best_common.astype(np.uint32)), "match and the detour differ"
    hit = best_common > 0
    assert np.array_equal(res.best[hit], best[hit].astype(np.uint32))
    match(); floor()
    t_match, t_floor = timed(match, reps), timed(floor, reps)
    t_match_small, t_detour = timed(lambda: match(nd), reps), timed(detour, max(1, min(reps, 2)))
    L = pkg.lib()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    full = match()
    L.smh_profile_enable(0)
    m, f, ms, d = (float(np.median(x)) for x in (t_match, t_floor, t_match_small, t_detour))
    return {
        "shape": name, "records": n_records, "record_len": record_len, "bytes": total,
        "records_with_a_hit": int((full.hit_distinct > 0).sum()), "sampled_windows": int(full.windows.sum(dtype=np.uint64)),
        "match_s": t_match, "match_median_s": m, "one_sketch_s": t_floor, "one_sketch_median_s": f,
        "match_over_one_sketch": m / f if f else None,
        "detour_records": nd, "match_small_s": t_match_small, "detour_s": t_detour,
        "detour_over_match": d / ms if ms else None,
        "kernel_ms": {k: prof(k)[0] for k in ("dna_rolling", "match_probe", "match_tally")},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=60000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--contigs", type=int, default=2000)
    ap.add_argument("--contig-len", type=int, default=5000000)
    ap.add_argument("--sketches", type=int, default=10000)
    ap.add_argument("--hashes", type=int, default=5000)
    ap.add_argument("--planted", type=int, default=200)
    ap.add_argument("--detour-reads", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r14_bench_match.json"))
    a = ap.parse_args()

    t0 = time.perf_counter()
    nodes = []
    for i in range(a.sketches):
        mh = fresh()
        mh.add_many(np.unique(splitmix64(14_000_003 + i, np.arange(a.hashes, dtype=np.uint64)) >> np.uint64(10)))
        if i < a.planted:
            piece = stream_tensor(i * MBP, MBP)
            own = fresh()
            own.add_sequences_dev(piece.data_ptr(), MBP, np.array([0, MBP], dtype=np.uint64), True)
            mh.add_many(own.mins_np())
        nodes.append(mh)
    index = pkg.index.ResidentIndex(nodes)
    index.match([b"A" * KSIZE])      # builds the hash directory: not part of any timing below
    print("setup %.1f s: %d nodes" % (time.perf_counter() - t0, a.sketches), flush=True)

    lds_pairs, threads, samples = pkg.matrix.match_geometry()
    out = {"tool": "tools/bench_match.py", "ksize": KSIZE, "scaled": 1000, "sketches": a.sketches, "hashes_per_sketch": a.hashes,
           "planted_nodes": a.planted, "pair_budget": pkg.matrix.match_pair_budget(),
           "geometry": {"lds_pairs": lds_pairs, "threads_per_record": threads, "probe_samples": samples},
           "shapes": [shape(index, "reads", a.reads, a.read_len, a.reps, a.detour_reads),
                      shape(index, "contigs", a.contigs, a.contig_len, a.reps, min(a.detour_reads, 50))]}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
