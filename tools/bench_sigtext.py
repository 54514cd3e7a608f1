"""Signature JSON written on the device on one GPU: writes profiles/r25_bench_sigtext.json.

    python tools/bench_sigtext.py [--host-seconds 60] [--max-sketches 200000] [--kernel-nodes 200000] [--out profiles/r25_bench_sigtext.json]

Input: the index of tools/bench_sigscan.py -- synth.family_signatures, bottom-2000 sketches, k = 31, named "synthetic <i>" --
built from host sketches.  Its size is chosen from a timed sample so that the parent commit's route takes about --host-seconds,
but at most --max-sketches (the host route holds every sketch and 40 KB of text per sketch in host memory); the size and
whether the cap cut it are recorded.  Whole calls, medians of 3, in turns, after both routes were asserted to give equal bytes:
(a) ResidentIndex.save_signatures(): the text formatted on the device, then copied to host bytes;
(b) the parent commit's route: sketches() + one Signature per sketch + signature.save_signatures;
(c) ResidentIndex.sigtext(): the same text left in HBM;
(d) ResidentIndex.md5sums() alone.
The kernels' rates are taken on --kernel-nodes nodes (the input's nodes repeated by select(), made on the device: what the
kernels do does not depend on whose hashes they are) by HIP events -- sigtext_measure, sigtext_scan, sigtext_emit, sigtext_md5
-- and set against the traffic floor: hashes read three times, abundances twice, text written once, 16 B per node back, at
6.3 TB/s.  Last, one node of 5 M scaled hashes alone: the md5 chain of a single wave."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.3e12          # bytes / s, measured streaming rate of the part
RUNS = 3
NUM = 2000
SAMPLE = 1000
TIMERS = ("sigtext_measure", "sigtext_scan", "sigtext_emit", "sigtext_md5")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-seconds", type=float, default=60.0, help="what the parent's route should take on the input (default 60)")
    ap.add_argument("--max-sketches", type=int, default=200000, help="cap on the input's size (default 200000)")
    ap.add_argument("--kernel-nodes", type=int, default=200000, help="nodes of the index the kernel rates are taken on (default 200000)")
    ap.add_argument("--lone-hashes", type=int, default=5000000, help="hashes of the single scaled node (default 5 M)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_bench_sigtext.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    from sourmash_rust_amd import signature as sg, synth
    L = pkg.lib()

    def sketches(lo, hi):
        out = []
        for row in synth.family_signatures(lo, hi, num=NUM):
            mh = pkg.KmerMinHash(NUM, 31)
            mh.add_many(row)
            out.append(mh)
        return out

    def parent_route(idx, names):
        sigs = []
        for mh, name in zip(idx.sketches(), names):
            s = sg.Signature()
            s.name = name
            s.push_mh(mh)
            sigs.append(s)
        return sg.save_signatures(sigs).encode()

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def kernel_ms(fn):
        """per-call times of the four timers over RUNS calls of fn"""
        L.smh_profile_reset(); L.smh_profile_enable(1)
        wall = [timed(fn)[0] for _ in range(RUNS)]
        out = {}
        for name in TIMERS:
            ms, cnt = C.c_double(), C.c_uint64()
            L.smh_profile_get(name.encode(), C.byref(ms), C.byref(cnt))
            out[name] = ms.value / RUNS
        L.smh_profile_enable(0)
        return out, wall

    mhs = sketches(0, SAMPLE)
    names = ["synthetic %d" % i for i in range(SAMPLE)]
    sample = pkg.index.ResidentIndex(mhs)
    sample.save_signatures(names=names); parent_route(sample, names)                       # warm-up
    t_sample = timed(lambda: parent_route(sample, names))[0]
    wanted = SAMPLE * args.host_seconds / t_sample
    n = int(max(SAMPLE, min(args.max_sketches, wanted)))
    print("sample: %d sketches in %.2f s on the parent's route -> %d sketches (%d for %.0f s)" % (SAMPLE, t_sample, n, wanted, args.host_seconds),
          flush=True)
    mhs += sketches(SAMPLE, n)
    names = ["synthetic %d" % i for i in range(n)]
    idx = pkg.index.ResidentIndex(mhs)
    del mhs, sample
    text = idx.save_signatures(names=names)
    assert text == parent_route(idx, names), "the device text differs from the parent's route"
    text_bytes = len(text)
    del text

    routes = {"a_device_to_host_bytes": lambda: idx.save_signatures(names=names), "b_parent_sketches_save_signatures": lambda: parent_route(idx, names),
              "c_device_text_in_hbm": lambda: idx.sigtext(names=names), "d_md5sums_alone": idx.md5sums}
    times = {k: [] for k in routes}
    for _ in range(RUNS):                                            # in turns
        for name, fn in routes.items():
            times[name].append(timed(fn)[0])
        print({k: round(v[-1], 4) for k, v in times.items()}, flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}

    # the kernels on many nodes: the input's nodes repeated on the device
    many = idx.select(np.arange(args.kernel_nodes, dtype=np.int64) % n)
    many_names = [names[i % n] for i in range(args.kernel_nodes)]
    t = many.sigtext(names=many_names)
    many_text = len(t)
    del t
    hashes = args.kernel_nodes * NUM
    kern, wall = kernel_ms(lambda: many.sigtext(names=many_names))
    md5_alone, md5_wall = kernel_ms(many.md5sums)
    floor_s = (3 * 8 * hashes + many_text + 16 * args.kernel_nodes) / COPY_RATE
    text_kernels_ms = kern["sigtext_measure"] + kern["sigtext_scan"] + kern["sigtext_emit"]
    del many

    # one node of millions: a single wave's chain
    rng = np.random.default_rng(7)
    lone_hashes = np.unique(rng.integers(0, 2 ** 63, size=args.lone_hashes + args.lone_hashes // 64, dtype=np.uint64))[:args.lone_hashes]
    mh = pkg.KmerMinHash(0, 31, False, 42, 2 ** 64 - 1)
    mh.add_many(lone_hashes)
    lone = pkg.index.ResidentIndex([mh])
    t = lone.sigtext()
    lone_text = len(t)
    del t
    assert lone.md5sums() == [hashlib.md5(("31" + "".join(map(str, lone_hashes.tolist()))).encode()).hexdigest()]
    lone_kern, lone_wall = kernel_ms(lone.sigtext)
    lone_digits = lone_text - (len(lone_hashes) - 1) - 300          # the text without its commas and (about) its skeleton

    result = {
        "sketches": n, "sketches_for_host_seconds": int(wanted), "host_seconds_wanted": args.host_seconds,
        "capped_by_max_sketches": wanted > args.max_sketches, "max_sketches": args.max_sketches, "hashes_per_sketch": NUM,
        "text_bytes": text_bytes, "runs": RUNS, "copy_rate_bytes_per_s": COPY_RATE,
        "calls_s": {k: spread(v) for k, v in times.items()}, "text_gb_per_s": {k: text_bytes / v / 1e9 for k, v in med.items()},
        "b_over_a": med["b_parent_sketches_save_signatures"] / med["a_device_to_host_bytes"],
        "b_over_c": med["b_parent_sketches_save_signatures"] / med["c_device_text_in_hbm"],
        "many_nodes": {
            "nodes": args.kernel_nodes, "hashes": hashes, "text_bytes": many_text, "call_s": spread(wall), "kernels_ms": kern,
            "md5sums_alone": {"call_s": spread(md5_wall), "sigtext_md5_ms": md5_alone["sigtext_md5"]},
            "text_kernels_ms": text_kernels_ms, "floor_ms": floor_s * 1e3, "text_kernels_share_of_floor": floor_s / (text_kernels_ms / 1e3),
            "text_kernels_gb_per_s_of_text": many_text / (text_kernels_ms / 1e3) / 1e9,
            "md5_gb_per_s_of_text": many_text / (kern["sigtext_md5"] / 1e3) / 1e9,
        },
        "one_node": {
            "hashes": int(len(lone_hashes)), "text_bytes": lone_text, "call_s": spread(lone_wall), "kernels_ms": lone_kern,
            "md5_mb_per_s_of_digits": lone_digits / (lone_kern["sigtext_md5"] / 1e3) / 1e6,
        },
    }
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
