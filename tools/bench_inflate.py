"""Blocked gzip inflated on the device on one GPU: writes profiles/r23_bench_inflate.json.

    python tools/bench_inflate.py [--gib 1] [--out profiles/r23_bench_inflate.json] [--no-trace]

Input: `--gib` GiB of FASTQ text (150-base reads, synthetic bases and qualities) and as much 80-column FASTA, each compressed
to BGZF at level 6 (65 280-byte blocks) with a 16-thread pool.  Per input, whole calls, medians of 3, in turns, after the
four routes were asserted to give equal bytes:
(a) fastx.inflate(host bytes): the compressed bytes are uploaded, then inflated on the device;
(b) today's route: gzip.decompress on one core, then the text is uploaded;
(c) the fair host route: zlib.decompressobj(-15) per member over a 16-thread pool (zlib releases the GIL), then upload;
(d) a plain upload of the uncompressed text: the link floor.
Kernel time by HIP events (profile name inflate) with verify on and off, as GB/s of text out and as a share of the traffic
floor (compressed bytes read + text written, + the text read once more for the CRC) / 6.3 TB/s; per kernel from a
`rocprofv3 --kernel-trace --stats` run of its own.  End to end: BGZF file -> read_device_text -> Records.parse -> add_records
against read_text -> Records.parse -> add_records.  The driver process starts the measuring process (and the traced one) as
children and never opens the GPU itself."""
import argparse
import csv
import ctypes as C
import glob
import gzip
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.3e12          # bytes / s, measured streaming rate of the part
RUNS = 3
BLOCK = 65280
THREADS = 16


def fastq_text(np, nbytes, read=150):
    rng = np.random.default_rng(4)
    rec = 12 + (read + 1) + 2 + (read + 1)
    n = max(1, nbytes // rec)
    t = np.empty((n, rec), dtype=np.uint8)
    idx = np.arange(n, dtype=np.int64)
    t[:, 0] = 0x40
    for d in range(10):
        t[:, 10 - d] = (idx // 10 ** d) % 10 + 48
    t[:, 11] = 0x0A
    t[:, 12:12 + read] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, read), dtype=np.uint8)]
    t[:, 12 + read] = 0x0A
    t[:, 13 + read] = 0x2B
    t[:, 14 + read] = 0x0A
    # qualities the way binned instruments write them: four values, mostly the best
    t[:, 15 + read:15 + 2 * read] = np.frombuffer(b"FFFFFF:,", dtype=np.uint8)[rng.integers(0, 8, (n, read), dtype=np.uint8)]
    t[:, 15 + 2 * read] = 0x0A
    return t.tobytes()


def fasta_text(np, nbytes, width=80, rec_lines=62500):
    rng = np.random.default_rng(5)
    per = 12 + rec_lines * (width + 1)
    n = max(1, nbytes // per)
    if nbytes < per:
        rec_lines, n = max(1, (nbytes - 12) // (width + 1)), 1
        per = 12 + rec_lines * (width + 1)
    t = np.empty((n, per), dtype=np.uint8)
    t[:, :12] = np.frombuffer(b"".join(b">chr%07d\n" % i for i in range(n)), dtype=np.uint8).reshape(n, 12)
    body = t[:, 12:].reshape(n, rec_lines, width + 1)
    body[:, :, :width] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, rec_lines, width), dtype=np.uint8)]
    body[:, :, width] = 0x0A
    return t.tobytes()


def bgzf_member(block):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = c.compress(block) + c.flush()
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(payload) + 25) + payload + \
        struct.pack("<II", zlib.crc32(block), len(block))


def bgzf(text, pool):
    view = memoryview(text)
    return b"".join(pool.map(bgzf_member, [view[i:i + BLOCK] for i in range(0, len(text), BLOCK)])) + bgzf_member(b"")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def prof(L, name):
    ms, cnt = C.c_double(), C.c_uint64()
    L.smh_profile_get(name, C.byref(ms), C.byref(cnt))
    return ms.value, cnt.value


def measure(args):
    import warnings
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    warnings.filterwarnings("ignore", message=".*not writable.*")    # (the uploads read host bytes in place)
    pkg = load_package()
    fx, L = pkg.fastx, pkg.lib()
    nbytes = int(args.gib * (1 << 30))
    pool = ThreadPoolExecutor(THREADS)
    result = {"gib_of_text": args.gib, "runs": RUNS, "copy_rate_bytes_per_s": COPY_RATE, "block": BLOCK, "threads": THREADS, "inputs": {}}
    tmp = tempfile.mkdtemp(prefix="bench_inflate_")
    for fmt, make in (("fastq", fastq_text), ("fasta", fasta_text)):
        text = make(np, nbytes)
        t0 = time.perf_counter()
        data = bgzf(text, pool)
        print("%s: %d text bytes, %d compressed, packed in %.1f s" % (fmt, len(text), len(data), time.perf_counter() - t0), flush=True)
        members = fx.gzip_scan(data)
        spans = [members.member(i)[:2] for i in range(len(members))]

        def upload(b):
            return torch.from_numpy(np.frombuffer(b, dtype=np.uint8)).cuda()

        def route_a():
            return fx.inflate(data)

        def route_b():
            return upload(gzip.decompress(data))

        def route_c():
            parts = pool.map(lambda s: zlib.decompressobj(-15).decompress(data[s[0]:s[0] + s[1]]), spans)
            return upload(b"".join(parts))

        def route_d():
            return upload(text)

        def timed(fn):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        routes = {"a_device_inflate": route_a, "b_gzip_one_core": route_b, "c_zlib_16_threads": route_c, "d_upload_text": route_d}
        ref = upload(text)
        for name, fn in routes.items():                              # warm-up, and equal bytes first
            assert torch.equal(fn(), ref), name
        comp = upload(data)
        if args.trace_child:
            fx.inflate(comp, members=members, verify=True)
            fx.inflate(comp, members=members, verify=False)
            continue
        times = {name: [] for name in routes}
        for _ in range(RUNS):                                        # in turns
            for name, fn in routes.items():
                times[name].append(timed(fn)[0])
            print(fmt, {k: round(v[-1], 3) for k, v in times.items()}, flush=True)
        kernel = {}
        for verify in (True, False):
            L.smh_profile_reset(); L.smh_profile_enable(1)
            for _ in range(RUNS):
                fx.inflate(comp, members=members, verify=verify)
            ms, n = prof(L, b"inflate")
            L.smh_profile_enable(0)
            floor = (len(data) + len(text) * (2 if verify else 1)) / COPY_RATE
            kernel["verify_on" if verify else "verify_off"] = {"ms": ms / n, "text_gb_per_s": len(text) / (ms / n / 1e3) / 1e9,
                                                               "floor_ms": floor * 1e3, "share_of_floor": floor / (ms / n / 1e3)}
        # end to end, from files
        bg = os.path.join(tmp, fmt + ".bgz")
        with open(bg, "wb") as fh:
            fh.write(data)
        mx = (1 << 64) // 1000

        def e2e_device():
            mh = pkg.KmerMinHash(0, 31, False, 42, mx, True)
            mh.add_records(fx.Records.parse(fx.read_device_text(bg)), True)
            return mh

        def e2e_host():
            mh = pkg.KmerMinHash(0, 31, False, 42, mx, True)
            mh.add_records(fx.Records.parse(fx.read_text(bg)), True)
            return mh

        a, b = e2e_device(), e2e_host()
        assert np.array_equal(a.mins_np(), b.mins_np()) and np.array_equal(a.abunds_np(), b.abunds_np())
        e2e = {"read_device_text": [], "read_text": []}
        for _ in range(RUNS):
            e2e["read_device_text"].append(timed(e2e_device)[0])
            e2e["read_text"].append(timed(e2e_host)[0])
        os.remove(bg)
        med = {k: statistics.median(v) for k, v in times.items()}
        result["inputs"][fmt] = {
            "text_bytes": len(text), "compressed_bytes": len(data), "members": len(members), "ratio": len(text) / len(data),
            "calls_s": {k: spread(v) for k, v in times.items()},
            "text_gb_per_s": {k: len(text) / v / 1e9 for k, v in med.items()},
            "a_over_c": med["a_device_inflate"] / med["c_zlib_16_threads"], "a_over_b": med["a_device_inflate"] / med["b_gzip_one_core"],
            "kernel": kernel,
            "file_to_sketch_s": {k: spread(v) for k, v in e2e.items()},
        }
        del ref, comp, a, b, text, data
        torch.cuda.empty_cache()
        L.smh_release_workspace()
    os.rmdir(tmp)
    print("BENCH_INFLATE " + json.dumps(result))


def kernel_stats(directory):
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                if "k_inflate" in row["Name"]:
                    out["k_inflate"] = {"calls": int(row["Calls"]), "total_ms": int(row["TotalDurationNs"]) / 1e6,
                                        "average_ms": float(row["AverageNs"]) / 1e6}
    return out


def child(extra, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + extra
    p = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = []
    for ln in p.stdout:                                              # progress is passed on as it comes
        lines.append(ln)
        if not ln.startswith("BENCH_INFLATE "):
            sys.stderr.write(ln); sys.stderr.flush()
    if p.wait() != 0:
        raise SystemExit("child failed: %s (exit %d)" % (" ".join(cmd), p.returncode))
    return "".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_bench_inflate.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--measure-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.measure_child or args.trace_child:
        return measure(args)
    out = child(["--measure-child", "--gib", str(args.gib)])
    line = [ln for ln in out.splitlines() if ln.startswith("BENCH_INFLATE ")][-1]
    result = json.loads(line[len("BENCH_INFLATE "):])
    if not args.no_trace:
        with tempfile.TemporaryDirectory() as d:
            child(["--trace-child", "--gib", str(min(args.gib, 0.25))],
                  prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"])
            result["kernel_trace_at_quarter_gib"] = kernel_stats(d)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
