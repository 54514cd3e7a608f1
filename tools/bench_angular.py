"""Angular similarity matrix of a resident collection against the count matrix of the same collection.

Input: N splitmix64 sketches of about 2 000 hashes (synth.family_signatures), abundances 1..50 from the same generator, once
as 50 families and once as one family.  Per collection, in turns (angular with the prune pass, angular without it,
ResidentIndex.compare for count_common), REPS rounds after one warm-up round:
  kernel_ms   HIP events of the library around its kernels (smh_profile_get): "angular_block", and the compare kernels
  call_ms     host clock around the whole call, which ends in a device synchronise and includes the copy of the N x N
              output to the host
Before any timing `dot` is checked against a numpy recomputation on 200 sampled rows.  A sweep over small blocks (with and
without the prune pass) shows where the pass starts to pay: the library's threshold is chosen from it.

  python tools/bench_angular.py [N] [REPS] [OUT.json]      (default 10000 5 profiles/r11_bench_angular.json)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first, so that one HIP runtime is shared)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
from sourmash_rust_amd import synth  # noqa: E402

L = pkg.lib()
NEVER = (1 << 64) - 1
COMPARE_KERNELS = ("compare_wave", "compare_few", "compare_pair", "compare_fill", "compare_comp", "compare_tiled")


def prof(names):
    tot = 0.0
    for n in names:
        ms, k = C.c_double(), C.c_uint64()
        L.smh_profile_get(n.encode(), C.byref(ms), C.byref(k))
        tot += ms.value
    return tot


def collection(n, n_families):
    sigs = synth.family_signatures(0, n, num=2000, n_families=n_families)
    with np.errstate(over="ignore"):      # 1..50, different for the same hash in different sketches
        ab = (synth.splitmix64(99, sigs.reshape(-1)).reshape(sigs.shape) + np.arange(n, dtype=np.uint64)[:, None] * np.uint64(7)) % np.uint64(50) + np.uint64(1)
    ab[:, -1] = 1      # the largest hash fills the bottom-2000 sketch: its repeats are ignored (quirk Q3), the sketch holds 1
    nodes = []
    for i in range(n):
        mh = pkg.KmerMinHash(2000, 21, False, 42, 0, True)
        h, a = np.ascontiguousarray(sigs[i]), np.ascontiguousarray(ab[i])
        assert L.smh_add_many_with_abund(mh._p, h.ctypes.data_as(pkg._lib.u64p), a.ctypes.data_as(pkg._lib.u64p), h.size) == 0
        nodes.append(mh)
    return sigs, ab, nodes


def check_rows(sigs, ab, dot, rows):
    """dot of the sampled rows against every column, recomputed with numpy from the pooled hashes sorted once"""
    n, num = sigs.shape
    order = np.argsort(sigs.reshape(-1), kind="stable")
    sh = sigs.reshape(-1)[order]
    sa = ab.reshape(-1)[order]
    scol = (order // num).astype(np.int64)            # a hash sits once in a sketch: the columns of one hash are distinct
    for r in rows:
        lo = np.searchsorted(sh, sigs[r], "left")
        hi = np.searchsorted(sh, sigs[r], "right")
        exp = np.zeros(n, dtype=np.uint64)
        for k in range(num):
            exp[scol[lo[k]:hi[k]]] += ab[r, k] * sa[lo[k]:hi[k]]
        assert np.array_equal(exp, dot[r]), "dot differs from the numpy recomputation in row %d" % r


def timed(fn, kernels):
    L.smh_profile_reset()
    t0 = time.perf_counter()
    fn()
    return {"call_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": prof(kernels)}


def median(runs, key):
    return float(np.median([r[key] for r in runs]))


def bench_collection(n, n_families, reps):
    sigs, ab, nodes = collection(n, n_families)
    index = pkg.index.ResidentIndex(nodes)
    assert index.has_abundances
    L.smh_angular_set_prune_min_pairs(0)
    dot = index.angular_matrix(want=("dot",))["dot"]
    walked, skipped = pkg.matrix.angular_last_stats()
    rng = np.random.default_rng(1)
    check_rows(sigs, ab, dot, rng.choice(n, min(200, n), replace=False))
    L.smh_angular_set_prune_min_pairs(NEVER)
    plain = index.angular_matrix(want=("dot",))["dot"]
    assert np.array_equal(plain, dot), "the prune pass changed the result"
    walked_plain, _ = pkg.matrix.angular_last_stats()
    del plain, dot
    L.smh_profile_enable(1)
    variants = {
        "angular_pruned": (0, lambda: index.angular_matrix(want=("angular",)), ("angular_block",) + COMPARE_KERNELS),
        "angular_unpruned": (NEVER, lambda: index.angular_matrix(want=("angular",)), ("angular_block",)),
        "count_common": (0, lambda: index.compare(index, want=("count_common",)), COMPARE_KERNELS),
    }
    runs = {k: [] for k in variants}
    for rep in range(reps + 1):
        for name, (prune, fn, kernels) in variants.items():
            L.smh_angular_set_prune_min_pairs(prune)
            r = timed(fn, kernels)
            if name == "angular_pruned":
                r["angular_block_ms"] = prof(("angular_block",))
            if rep:
                runs[name].append(r)
    L.smh_angular_set_prune_min_pairs(0)
    L.smh_profile_enable(0)
    out = {"n": n, "n_families": n_families, "hashes_per_sketch": int(sigs.shape[1]), "pairs_walked_pruned": walked,
           "pairs_skipped_pruned": skipped, "pairs_walked_unpruned": walked_plain, "rows_checked_against_numpy": min(200, n)}
    for name in variants:
        out[name] = {"kernel_ms_median": median(runs[name], "kernel_ms"), "call_ms_median": median(runs[name], "call_ms"),
                     "kernel_ms_all": [round(r["kernel_ms"], 4) for r in runs[name]]}
    out["angular_pruned"]["angular_block_ms_median"] = median(runs["angular_pruned"], "angular_block_ms")
    out["angular_pruned_over_count_common_kernel"] = out["angular_pruned"]["kernel_ms_median"] / max(out["count_common"]["kernel_ms_median"], 1e-9)
    out["angular_unpruned_over_count_common_kernel"] = out["angular_unpruned"]["kernel_ms_median"] / max(out["count_common"]["kernel_ms_median"], 1e-9)
    return out


def sweep(reps):
    """small blocks of two different indexes (no cached dictionary): whole-call time with and without the prune pass"""
    out = []
    _, _, nodes = collection(1000, 50)
    L.smh_profile_enable(1)
    for n in (16, 32, 64, 100, 200, 400, 1000):
        a, b = pkg.index.ResidentIndex(nodes[:n]), pkg.index.ResidentIndex(nodes[:n])
        row = {"n": n, "pairs": n * n}
        for form, other in (("two_indexes", b), ("one_index", None)):
            for name, prune in (("pruned", 1), ("unpruned", NEVER)):
                L.smh_angular_set_prune_min_pairs(prune)
                rs = []
                for rep in range(reps + 2):
                    r = timed(lambda: a.angular_matrix(other, want=("angular",)), ("angular_block",) + COMPARE_KERNELS)
                    if rep >= 2:
                        rs.append(r)
                row["%s_%s_call_ms" % (form, name)] = median(rs, "call_ms")
                row["%s_%s_kernel_ms" % (form, name)] = median(rs, "kernel_ms")
            row["%s_walked" % form] = pkg.matrix.angular_last_stats()[0]
        out.append(row)
    L.smh_angular_set_prune_min_pairs(0)
    L.smh_profile_enable(0)
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r11_bench_angular.json")
    assert torch.cuda.is_available(), "bench_angular needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "default_prune_min_pairs": int(L.smh_angular_prune_min_pairs()),
           "reps": reps, "prune_sweep_1000_sketches_50_families": sweep(max(reps, 5))}
    print(json.dumps(res["prune_sweep_1000_sketches_50_families"]), flush=True)
    for fam, key in ((50, "families_50"), (1, "one_family")):
        res[key] = bench_collection(n, fam, reps)
        print(key, json.dumps(res[key]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
