"""Taxonomic LCA on a resident index next to what a caller had before it.

    python tools/bench_lca.py [--reads 60000000] [--read-len 150] [--sketches 10000] [--hashes 5000] [--planted 200]
                              [--detour-reads 20000] [--gm-sketches 20000] [--queries 64] [--reps 3]
                              [--out profiles/r16_bench_lca.json]

Records route: the index and the read batch of tools/bench_match.py, with a synthetic taxonomy over the nodes (a tree of
`--taxa` taxa, parent[t] = a splitmix64 pick among the 64 taxa in front of t; node i sits at taxon splitmix64 pick, every
97th node has no lineage).  lca_classify_records is timed in turns with (a) match of the same batch on the same index and
(b) the detour on a slice: match(hits=True), the hit hashes back on the host, the owner lists and lineages walked in Python.
The detour and the device are asserted equal on the slice before anything is timed.
Sketch route: the index and the query batch of tools/bench_gather_many.py; lca_counts of the batch next to gather_many's probe
phase of the same batch (its timer gather_many_probe; ours: lca_probe), and the whole lca_counts call.
Medians of `reps` whole calls, wall clock around calls that return with their device work complete; kernel shares from a
separate run under smh_profile_enable.  No ratio is claimed in advance: the figures are what the file says.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_match as BM  # noqa: E402  (the index pieces, stream_tensor, prof; loads the package)

pkg = BM.pkg
from sourmash_rust_amd.synth import splitmix64  # noqa: E402

NO = pkg.index.NO_TAXON


def taxonomy(n_taxa, n_nodes):
    t = np.arange(n_taxa, dtype=np.uint64)
    back = splitmix64(16_000_001, t) % np.uint64(64) + np.uint64(1)
    parent = np.where(t > back, t - back, 0).astype(np.uint32)
    parent[0] = 0
    node_taxon = (splitmix64(16_000_002, np.arange(n_nodes, dtype=np.uint64)) % np.uint64(n_taxa)).astype(np.uint32)
    node_taxon[::97] = NO
    return parent, node_taxon


def host_lca(parent, node_taxon, owners, res):
    """the detour's host half: per record the literal rule on the hit hashes match returned; owners = (hashes ascending,
    the node holding each)"""
    taxon, status = np.full(len(res.windows), NO, dtype=np.uint32), np.zeros(len(res.windows), dtype=np.uint32)
    memo = {}

    def path(t):
        out = [t]
        while t:
            t = int(parent[t]); out.append(t)
        return out[::-1]

    def lca(a, b):
        pa, pb = path(a), path(b)
        k = 0
        while k < min(len(pa), len(pb)) and pa[k] == pb[k]:
            k += 1
        return pa[k - 1]

    all_h, all_n = owners
    for r in range(len(res.windows)):
        taxa = set()
        for h in res.hit_hashes[int(res.hit_offsets[r]):int(res.hit_offsets[r + 1])].tolist():
            t = memo.get(h)
            if t is None:
                t = NO
                for node in all_n[np.searchsorted(all_h, h, "left"):np.searchsorted(all_h, h, "right")].tolist():
                    nt = int(node_taxon[node])
                    if nt != NO:
                        t = nt if t == NO else lca(t, nt)
                memo[h] = t
            if t != NO:
                taxa.add(t)
        if taxa:
            taxon[r], status[r] = pkg.index.lca_classify(parent, sorted(taxa), [1] * len(taxa), 1)
    return taxon, status


def timed_in_turns(fns, reps):
    out = [[] for _ in fns]
    for _ in range(reps):     # in turns: other people's work shares the machine
        for k, fn in enumerate(fns):
            t0 = time.perf_counter(); fn(); out[k].append(time.perf_counter() - t0)
    return out


def records_route(a):
    nodes = []
    for i in range(a.sketches):
        mh = BM.fresh()
        mh.add_many(np.unique(splitmix64(14_000_003 + i, np.arange(a.hashes, dtype=np.uint64)) >> np.uint64(10)))
        if i < a.planted:
            piece = BM.stream_tensor(i * BM.MBP, BM.MBP)
            own = BM.fresh()
            own.add_sequences_dev(piece.data_ptr(), BM.MBP, np.array([0, BM.MBP], dtype=np.uint64), True)
            mh.add_many(own.mins_np())
        nodes.append(mh)
        if (i + 1) % 1000 == 0:
            print("records route: %d nodes made" % (i + 1), flush=True)
    index = pkg.index.ResidentIndex(nodes)
    parent, node_taxon = taxonomy(a.taxa, a.sketches)
    index.set_taxonomy(parent, node_taxon)
    total = a.reads * a.read_len
    seq = BM.stream_tensor(0, total)
    off = np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(a.read_len)
    nd = min(a.detour_reads, a.reads)

    def batch(n):
        return (seq.data_ptr(), n * a.read_len, off[:n + 1])

    # the owner lists "pulled back": every (hash, node) pair sorted by hash, on the host (made once, outside the timings)
    mins = [mh.mins_np() for mh in nodes]
    all_h = np.concatenate(mins)
    all_n = np.repeat(np.arange(len(nodes), dtype=np.uint32), [m.size for m in mins])
    order = np.argsort(all_h, kind="stable")
    owners = (all_h[order], all_n[order])
    print("records route: index, batch and owner arrays ready", flush=True)
    small = index.lca_classify_records(batch(nd))     # builds the directory and the table: not part of any timing below
    taxon, status = host_lca(parent, node_taxon, owners, index.match(batch(nd), hits=True))
    assert np.array_equal(small.taxon, taxon) and np.array_equal(small.status, status), "the device and the detour differ"
    index.lca_classify_records(batch(a.reads)); index.match(batch(a.reads))
    t_lca, t_match = timed_in_turns([lambda: index.lca_classify_records(batch(a.reads)), lambda: index.match(batch(a.reads))], a.reps)
    t_small, t_detour = timed_in_turns([lambda: index.lca_classify_records(batch(nd)),
                                        lambda: host_lca(parent, node_taxon, owners, index.match(batch(nd), hits=True))], a.reps)
    L = pkg.lib()
    timers = {}
    for what, fn in (("lca", lambda: index.lca_classify_records(batch(a.reads))), ("match", lambda: index.match(batch(a.reads)))):
        L.smh_profile_reset(); L.smh_profile_enable(1)
        full = fn()
        L.smh_profile_enable(0)
        timers[what] = {k: BM.prof(k)[0] for k in ("dna_rolling", "match_probe", "match_tally", "lca_records")}
    full = index.lca_classify_records(batch(a.reads))
    m_lca, m_match, m_small, m_detour = (float(np.median(x)) for x in (t_lca, t_match, t_small, t_detour))
    return {"reads": a.reads, "read_len": a.read_len, "sketches": a.sketches, "taxa": a.taxa,
            "status_counts": np.bincount(full.status, minlength=3).tolist(),
            "lca_s": t_lca, "lca_median_s": m_lca, "match_s": t_match, "match_median_s": m_match, "lca_over_match": m_lca / m_match,
            "detour_reads": nd, "lca_small_s": t_small, "detour_s": t_detour, "detour_over_lca": m_detour / m_small if m_small else None,
            "kernel_ms": timers}


def sketch_route(a):
    import bench_gather as BG
    import bench_gather_many as BGM
    sketches = BG.make_sketches(a.gm_sketches)
    every = np.unique(np.concatenate(sketches))
    index = pkg.index.ResidentIndex([BG.sketch_of(s) for s in sketches])
    parent, node_taxon = taxonomy(a.taxa, a.gm_sketches)
    index.set_taxonomy(parent, node_taxon)
    print("sketch route: index of %d sketches made" % a.gm_sketches, flush=True)
    queries = []
    for q in range(a.queries):
        queries.append(BG.sketch_of(BGM.make_query(q, sketches, every)[0]))
        if (q + 1) % 8 == 0:
            print("sketch route: %d queries made" % (q + 1), flush=True)
    index.lca_counts(queries)
    kw = dict(threshold_bp=1, scaled=1, abund_stats=False)
    index.gather_many(queries[:4], **kw)
    (t_lca,) = timed_in_turns([lambda: index.lca_counts(queries)], a.reps)
    L = pkg.lib()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    got = index.lca_counts(queries)
    index.gather_many(queries, **kw)
    L.smh_profile_enable(0)
    return {"sketches": a.gm_sketches, "queries": a.queries, "query_hashes_total": int(sum(len(q) for q in queries)),
            "pairs_total": int(sum(t.size for t, _ in got)), "lca_counts_s": t_lca, "lca_counts_median_s": float(np.median(t_lca)),
            "kernel_ms": {k: BM.prof(k)[0] for k in ("lca_probe", "gather_many_probe")}, "budget": pkg.matrix.lca_budget()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=60000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sketches", type=int, default=10000)
    ap.add_argument("--hashes", type=int, default=5000)
    ap.add_argument("--planted", type=int, default=200)
    ap.add_argument("--taxa", type=int, default=20000)
    ap.add_argument("--detour-reads", type=int, default=20000)
    ap.add_argument("--gm-sketches", type=int, default=20000)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r16_bench_lca.json"))
    a = ap.parse_args()
    owner_lane_max, record_lane_max, threads = pkg.matrix.lca_geometry()
    out = {"tool": "tools/bench_lca.py", "ksize": BM.KSIZE, "scaled": 1000,
           "geometry": {"owner_lane_max": owner_lane_max, "record_lane_max": record_lane_max, "threads": threads}}
    for name, fn in (("records", records_route), ("sketches", sketch_route)):
        t0 = time.perf_counter()
        out[name] = fn(a)
        print("%s route done in %.1f s: %s" % (name, time.perf_counter() - t0, json.dumps(out[name])), flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:     # after every route: a run cut short leaves what it measured
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
