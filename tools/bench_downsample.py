"""Downsampling a resident index on the device (smh_index_downsample) next to two yardsticks: what a caller could do before
it -- cut every sketch on the host and upload a new index -- and a plain device-to-device copy of the kept bytes.

    python tools/bench_downsample.py [--sketches 10000] [--hashes 20000] [--keep 0.1] [--reps 5] [--host-reps 2]
                                     [--out profiles/r13_bench_downsample.json]

Input (deterministic): sketch i holds the distinct values of splitmix64(11_000_003 + i, j) >> 10 for j < hashes, which lie
below max_hash = 2^64 // 1000 (scaled = 1000), ascending, no abundances.  The cut is at keep * max_hash.  The device cut
and the host route are asserted to give the same kept lengths before anything is timed.  All three are timed in turns, wall
clock around calls that return with their device work complete; the kernels' share comes from a separate run under
smh_profile_enable (HIP events).  No ratio is claimed in advance: the figures are what the file says.
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
from sourmash_rust_amd.synth import splitmix64  # noqa: E402

MAX_HASH = (1 << 64) // 1000


def prof(name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return ms.value, k.value


def sketch_of(hashes, max_hash):
    mh = pkg.KmerMinHash(0, 31, False, 42, max_hash, False)
    mh.add_many(hashes)
    return mh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=10000)
    ap.add_argument("--hashes", type=int, default=20000)
    ap.add_argument("--keep", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "r13_bench_downsample.json"))
    a = ap.parse_args()
    new_max = int(MAX_HASH * a.keep)

    t0 = time.perf_counter()
    arrays = [np.unique(splitmix64(11_000_003 + i, np.arange(a.hashes, dtype=np.uint64)) >> np.uint64(10)) for i in range(a.sketches)]
    nodes = [sketch_of(x, MAX_HASH) for x in arrays]
    index = pkg.index.ResidentIndex(nodes)
    total = int(sum(x.size for x in arrays))
    kept_lens = [int(np.searchsorted(x, np.uint64(new_max), side="right")) for x in arrays]
    kept = int(sum(kept_lens))
    print("setup %.1f s: %d sketches, %d resident hashes, %d kept at %.3f of max_hash" % (time.perf_counter() - t0, a.sketches, total, kept, a.keep),
          flush=True)

    def device_cut():
        index.drop_downsampled()
        return index.downsample(max_hash=new_max)

    def host_route():
        return pkg.index.ResidentIndex([m.downsample_max_hash(new_max) for m in nodes])

    src = torch.zeros(max(total, 1), dtype=torch.int64, device="cuda")
    dst = torch.empty(max(kept, 1), dtype=torch.int64, device="cuda")

    def plain_copy():
        dst.copy_(src[:max(kept, 1)])
        torch.cuda.synchronize()

    child, rebuilt = device_cut(), host_route()
    q = sketch_of(arrays[0][:kept_lens[0]], new_max)
    assert len(child) == len(rebuilt) == a.sketches and child.max_hash == rebuilt.max_hash == new_max
    cc_a = child.compare(pkg.index.ResidentIndex([q]), want=("count_common",))["count_common"]
    cc_b = rebuilt.compare(pkg.index.ResidentIndex([q]), want=("count_common",))["count_common"]
    assert np.array_equal(cc_a, cc_b) and int(cc_a[0, 0]) == kept_lens[0], "the device cut and the host route differ"
    del rebuilt
    plain_copy()

    t_dev, t_host, t_copy = [], [], []
    for k in range(max(a.reps, a.host_reps)):     # in turns: other people's work shares the host
        if k < a.reps:
            t0 = time.perf_counter(); device_cut(); t_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); plain_copy(); t_copy.append(time.perf_counter() - t0)
        if k < a.host_reps:
            t0 = time.perf_counter(); r = host_route(); t_host.append(time.perf_counter() - t0)
            del r

    L = pkg.lib()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    device_cut()
    L.smh_profile_enable(0)
    bounds_ms, _ = prof("downsample_bounds")
    copy_ms, _ = prof("downsample_copy")
    tile, threads = pkg.matrix.downsample_geometry()
    d, h, c = float(np.median(t_dev)), float(np.median(t_host)), float(np.median(t_copy))
    moved = 16 * kept   # the copy reads and writes every kept hash once
    out = {
        "tool": "tools/bench_downsample.py", "sketches": a.sketches, "resident_hashes": total, "kept_hashes": kept, "keep": a.keep,
        "tile_elems": tile, "threads": threads,
        "device_cut_s": t_dev, "device_cut_median_s": d,
        "host_route_s": t_host, "host_route_median_s": h,
        "plain_copy_s": t_copy, "plain_copy_median_s": c,
        "kernel_ms": {"downsample_bounds": bounds_ms, "downsample_copy": copy_ms},
        "copy_kernel_gb_per_s": moved / (copy_ms * 1e-3) / 1e9 if copy_ms else None,
        "plain_copy_gb_per_s": moved / c / 1e9 if c else None,
    }
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
