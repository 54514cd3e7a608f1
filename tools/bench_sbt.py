"""Row N5: SBT::find over a device-built tree of family leaves (C4-style: num = 2000, 50 families, leaves in family
order) against the resident linear scan (ResidentIndex.find) and the tests' restatement.  Two table sizes: the sourmash
default 4 x ~1e5 bits (LDS-staged node tests) and 4 x ~1e6 bits (gathered from global memory).
Run on the GPU box: python tools/bench_sbt.py [n_leaves] [n_queries]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402  (maps torch's HIP runtime first)
from __graft_entry__ import load_package  # noqa: E402
pkg = load_package()
from sourmash_rust_amd import synth  # noqa: E402
import sbt_restatement as R  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
nq = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
num, fams = 2000, 50
sigs = synth.family_signatures(0, n, num=num, n_families=fams, seed=3)
order = sorted(range(n), key=lambda i: (i % fams, i))          # leaves in family order
leaves = []
for i in order:
    m = pkg.KmerMinHash(num, 31, False, 42, 0)
    m.add_many(sigs[i])
    leaves.append(m)
rng = np.random.default_rng(7)
qidx = rng.choice(n, size=nq, replace=False)
queries = [leaves[i] for i in qidx]
L = pkg.lib()


def prof(names):
    out = {}
    for name in names:
        ms, cnt = C.c_double(), C.c_uint64()
        L.smh_profile_get(name.encode(), C.byref(ms), C.byref(cnt))
        out[name] = dict(ms=round(ms.value, 3), launches=cnt.value)
    return out


def primes_below(x, k):
    out, v = [], x - 1
    while len(out) < k:
        if v > 1 and all(v % p for p in range(2, int(v ** 0.5) + 1)):
            out.append(v)
        v -= 1
    return out


res = dict(n_leaves=n, n_queries=nq, num=num, families=fams, runs=[])
idx = pkg.index.ResidentIndex(leaves)
idx.find(queries[0], 0.1)
t0 = time.perf_counter()
lin = {}
for cont in (False, True):
    lin[cont] = [idx.find(q, 0.1, containment=cont) for q in queries[:200]]
t_lin = (time.perf_counter() - t0) / 400
res["resident_index_find_ms_per_query"] = round(t_lin * 1e3, 3)
for label, start in (("4x1e5", 100000), ("4x1e6", 1000000)):
    sizes = primes_below(start, 4)
    torch.cuda.synchronize()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    t0 = time.perf_counter()
    tree = pkg.SBT.build(leaves, sizes, ksize=31, d=2)
    t_build = time.perf_counter() - t0
    L.smh_profile_enable(0)
    build_prof = prof(["sbt_build"])
    tree.find_many(queries[:10], 0.1)   # warm the work space
    run = dict(tables=label, sizes=sizes, nodes=tree.n_nodes, table_bytes_per_node=sum((s + 63) // 64 * 8 for s in sizes),
               build_s=round(t_build, 3), build_kernels=build_prof)
    for cont in (False, True):
        L.smh_profile_reset(); L.smh_profile_enable(1)
        t0 = time.perf_counter()
        hits = tree.find_many(queries, 0.1, cont)
        dt = time.perf_counter() - t0
        L.smh_profile_enable(0)
        # the walk's work, restated on the host from the hits: node tests and leaf compares per query are what the
        # kernels launched (sbt_nodes / sbt_leaves launches are per level / per chunk, not per pair)
        k = prof(["sbt_bins", "sbt_nodes", "sbt_leaves"])
        # linear-scan parity for the first 200 queries: the tree's hits as a set equal the scan's
        pos = tree.leaf_positions()
        for qi in range(200):
            assert sorted(hits[qi]) == sorted(pos[j] for j in lin[cont][qi]), (label, cont, qi)
        run["containment" if cont else "similarity"] = dict(
            seconds=round(dt, 4), queries_per_s=round(nq / dt, 1), hits_per_query=round(sum(map(len, hits)) / nq, 2),
            kernels=k)
    res["runs"].append(run)
    del tree
# node tests / leaf compares per query at the default tables, from the restatement on a sample of queries
sizes = res["runs"][0]["sizes"]
pos = pkg.sbt.default_positions(n, 2)
lm = {p: sigs[i] for p, i in zip(pos, order)}
t0 = time.perf_counter()
nodes = R.build_nodes(2, {p: list(v) for p, v in lm.items()}, sizes)
t_rb = time.perf_counter() - t0
lv = {p: (list(v), num) for p, v in lm.items()}


def walk_counts(qmins, thr, cont):
    nt = lc = 0
    stack = [0]
    while stack:
        p = stack.pop()
        if p in nodes:
            nt += 1
            tables, mnb = nodes[p]
            m = R.matches(sizes, tables, qmins)
            v = m / len(qmins) if cont else m / mnb
            if v > thr:
                stack.extend(2 * p + c + 1 for c in range(2))
        elif p in lv:
            lc += 1
    return nt, lc


sample = [list(sigs[order[i]]) for i in qidx[:20]]
t0 = time.perf_counter()
counts = [walk_counts(q, 0.1, False) for q in sample]
t_py = (time.perf_counter() - t0) / len(sample)
res["restatement"] = dict(build_s=round(t_rb, 1), walk_s_per_query=round(t_py, 3),
                          node_tests_per_query=float(np.mean([c[0] for c in counts])),
                          leaf_compares_per_query=float(np.mean([c[1] for c in counts])))
print(json.dumps(res, indent=1))
