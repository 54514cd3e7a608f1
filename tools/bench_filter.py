"""Filtering a resident index on the device (smh_index_filter, smh_index_select) against what a caller did before it: every
sketch read back to the host, numpy set arithmetic per node, and a new index uploaded.

    python tools/bench_filter.py [--sketches 10000] [--families 50] [--reps 3] [--only subtract,select]
                                 [--out profiles/r21_bench_filter.json]

The index is the pairwise index of tools/bench_search_many.py (`--sketches` splitmix64 sketches of about 5 000 hashes in
`--families` families), here with abundances (1 + hash mod 5) so that every verb has something to carry.  The operand is the
union sketch of family 0, each hash weighted by the number of members that hold it.  The calls:

  subtract   index.subtract(operand)            the nodes without the operand's hashes, abundances kept
  intersect  index.intersect(operand)           the nodes restricted to the operand
  inflate    index.inflate(operand)             ... with the operand's abundances
  private    index.filter(min_owners=1, max_owners=1)    the hashes exactly one node holds
  window     index.filter(min_abund=2, max_abund=3)      an abundance window
  select     index.select(every tenth node)

The other route is index.sketches() + numpy (np.searchsorted of every node in the sorted operand; np.unique with counts over
all resident hashes and a searchsorted in it for the owners; a mask on the abundances) + ResidentIndex(...) of the new sketches.  As a floor, one device-to-device copy of the
bytes the child keeps (torch, HIP events).

Equal outputs (read() of both children) are asserted first.  Then the two routes are timed in turns, `reps` whole calls each
(the Python wrappers included), medians and the spread (max - min) reported.  filter_flag and filter_emit come from a run of
its own under smh_profile_enable (HIP events), and with them the bytes the two passes read and write, computed from the
shapes, per second.  The file is rewritten after every step: a run cut short leaves what it measured, and `--only` with the
same `--out` measures the named calls and keeps the others' runs as the file has them.  The host route takes many seconds per call at the
default size, so every timed call prints a line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bench_gather as BG  # noqa: E402  (h(), prof(), MAX_HASH; loads the package)
import bench_search_many as BS  # noqa: E402  (the pairwise index)
import bench_collapse as BC  # noqa: E402  (same(), spread(), copy_floor_ms(), dump())

pkg = BG.pkg
TIMERS = ("filter_flag", "filter_emit", "downsample_copy")
u64p = pkg.index.u64p


def weighted(hashes, abunds):
    mh = pkg.KmerMinHash(0, 31, False, 42, BG.MAX_HASH, True)
    if hashes.size:
        pkg.lib().smh_add_many_with_abund(mh._p, np.ascontiguousarray(hashes, dtype=np.uint64).ctypes.data_as(u64p),
                                          np.ascontiguousarray(abunds, dtype=np.uint64).ctypes.data_as(u64p), int(hashes.size))
    return mh


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


def host_route(index, what, op_h, op_a, ids):
    """the child index made on the host from the parent's sketches"""
    sk = index.sketches()
    if what == "select":
        return pkg.index.ResidentIndex([sk[i] for i in ids])
    mins = [s.mins_np() for s in sk]
    abunds = [s.abunds_np() for s in sk]
    if what == "private":
        table, count = np.unique(np.concatenate(mins), return_counts=True)
    else:
        table, count = op_h, None

    def found(m):
        """where every hash of m sits in the sorted table, and whether it is there"""
        at = np.minimum(np.searchsorted(table, m), table.size - 1)
        return at, table[at] == m

    made = []
    for m, a in zip(mins, abunds):
        if what == "window":
            keep = (a >= 2) & (a <= 3)
        else:
            at, there = found(m)
            keep = ~there if what == "subtract" else count[at] == 1 if what == "private" else there
        kept = m[keep]
        made.append(weighted(kept, op_a[at[keep]] if what == "inflate" else a[keep]))
    return pkg.index.ResidentIndex(made)


def turns(what, mine, theirs, reps):
    a, b = [], []
    for r in range(reps):     # in turns: other people's work shares the host
        t0 = time.perf_counter(); mine(); a.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); theirs(); b.append(time.perf_counter() - t0)
        print("  %s rep %d: device %.4f s, host route %.1f s" % (what, r, a[-1], b[-1]), flush=True)
    return a, b


def pass_bytes(what, total, kept, operand_len):
    """the bytes the flag and emit passes read and write, from the shapes: the hashes (8 B) or, for the abundance window, the
    abundances (4 B) of every resident hash in, one mask bit per hash out and in again, the survivors in and out; the searches' own traffic (the operand, the
    directory) is cached and not counted"""
    own = what in ("subtract", "intersect", "private", "window")
    # (a rule that is an abundance window alone never reads the hashes in the flag pass: 4 B per element)
    flag = (total * 4 if what == "window" else total * 8) + total // 8
    emit = total // 8 + kept * 8 * 2 + (kept * 4 * 2 if own else 0) + (kept * 4 if what == "inflate" else 0)
    return flag, emit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=10000)
    ap.add_argument("--families", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated calls to measure (default: all six)")
    ap.add_argument("--out", default=os.path.join("profiles", "r21_bench_filter.json"))
    a = ap.parse_args()
    tile, samples, threads = pkg.matrix.filter_geometry()
    n = a.sketches
    t0 = time.perf_counter()
    sketches = BS.make_family_sketches(n, a.families)
    index = pkg.index.ResidentIndex([weighted(s, 1 + s % np.uint64(5)) for s in sketches])
    total = int(index.sizes().sum())
    op_h, op_a = np.unique(np.concatenate(sketches[::a.families]), return_counts=True)
    operand = weighted(op_h, op_a)
    op_a = op_a.astype(np.uint64)
    ids = list(range(0, n, 10))
    print("index %.1f s: %d sketches in %d families, %d resident hashes, operand of %d" % (time.perf_counter() - t0, n, a.families, total, op_h.size),
          flush=True)
    out = {"tool": "tools/bench_filter.py", "sketches": n, "families": a.families, "resident_hashes": total, "operand_hashes": int(op_h.size),
           "reps": a.reps, "geometry": {"tile": tile, "operand_samples": samples, "threads": threads}, "runs": []}
    t0 = time.perf_counter()
    index.filter(max_owners=1)     # builds the hash directory, which the index keeps: not part of any timed call
    out["first_call_with_directory_s"] = time.perf_counter() - t0
    calls = [("subtract", lambda: index.subtract(operand)), ("intersect", lambda: index.intersect(operand)),
             ("inflate", lambda: index.inflate(operand)), ("private", lambda: index.filter(min_owners=1, max_owners=1)),
             ("window", lambda: index.filter(min_abund=2, max_abund=3)), ("select", lambda: index.select(ids))]
    only = [w for w in a.only.split(",") if w]
    if only and os.path.exists(a.out):     # continue a run: keep what the file has of the other calls
        with open(a.out) as fh:
            out["runs"] = [r for r in json.load(fh).get("runs", []) if r["what"] not in only]
    for what, dev in calls:
        if only and what not in only:
            continue

        def host():
            return host_route(index, what, op_h, op_a, ids)

        child = dev()
        assert BC.same(child, host()), "the device and the host route differ: %s" % what
        print("  %s: equal outputs" % what, flush=True)
        t_dev, t_host = turns(what, dev, host, a.reps)
        kept = int(child.sizes().sum())
        kept_bytes = kept * (12 if child.has_abundances else 8)
        run = {"what": what, "child_hashes": kept, "device": BC.spread(t_dev), "host_route": BC.spread(t_host),
               "ratio_host_over_device": float(np.median(t_host) / np.median(t_dev)), "timers": profiled(dev),
               "copy_floor_ms": BC.copy_floor_ms(max(kept_bytes, 8), a.reps), "kept_bytes": kept_bytes}
        if what != "select":
            fb, eb = pass_bytes(what, total, kept, int(op_h.size))
            run["bytes"] = {"filter_flag": fb, "filter_emit": eb}
            ms = run["timers"]["filter_flag"]["ms"] + run["timers"]["filter_emit"]["ms"]
            run["GB_per_s_flag_and_emit"] = float((fb + eb) / (ms * 1e-3) / 1e9) if ms else None
        del child
        print("%s: %s" % (what, json.dumps(run)), flush=True)
        out["runs"].append(run)
        BC.dump(out, a.out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
