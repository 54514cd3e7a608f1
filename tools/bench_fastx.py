"""The device FASTA / FASTQ parser on one GPU: writes profiles/r09_bench_fastx.json.

    python tools/bench_fastx.py [--gb 10] [--out profiles/r09_bench_fastx.json] [--no-trace]

(a) parse time of `--gb` GB of bases as FASTA (80 columns, 5 Mbp records) and as FASTQ (150-base reads): whole call,
    the two kernel groups by HIP events, and per kernel from a `rocprofv3 --kernel-trace --stats` run of its own;
    GB/s of text and the share of the floor (2 x text + kept bytes) / 6.3 TB/s;
(b) parse + add_records end to end against smh_add_sequences_dev on the same records already cut, the two alternating
    in one process;
(c) the read-back of the offsets at 28 M records, on its own.
Every figure is taken after a warm-up, three runs each, alternating.  The driver process starts the measuring process
(and the traced one) as children and never opens the GPU itself.  Also asserts, on the FASTA input, what the suite's
past-4-GiB test asserts: counts, offsets and the first and last bytes of the compacted buffer."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.3e12          # bytes / s, measured streaming rate of the part
RUNS = 3


def fasta_on_device(torch, L, n_bases, width=80, rec_bases=5_000_000):
    """bases as wrapped FASTA: records of rec_bases with a 12-byte header line.  Returns (text, bases, offsets)."""
    import numpy as np
    lines_per = rec_bases // width
    n_rec = max(1, n_bases // (lines_per * width))
    bases = torch.empty(n_rec * lines_per * width, dtype=torch.uint8, device="cuda")
    L.smh_synth_dna_dev(C.c_void_p(bases.data_ptr()), 0, bases.numel(), 3, 0, C.c_void_p(0))
    torch.cuda.synchronize()
    text = torch.empty((n_rec, 12 + lines_per * (width + 1)), dtype=torch.uint8, device="cuda")
    heads = np.frombuffer(b"".join(b">chr%07d\n" % i for i in range(n_rec)), dtype=np.uint8).reshape(n_rec, 12)
    text[:, :12] = torch.from_numpy(heads.copy()).cuda()
    body = text[:, 12:].view(n_rec, lines_per, width + 1)
    body[:, :, :width] = bases.view(n_rec, lines_per, width)
    body[:, :, width] = 0x0A
    off = np.arange(n_rec + 1, dtype=np.uint64) * np.uint64(lines_per * width)
    return text.view(-1), bases, off


def fastq_on_device(torch, L, n_bases, read=150):
    """'@' + 10 digits, the read, '+', a quality line of the read's length that begins with '@'."""
    import numpy as np
    n_rec = max(1, n_bases // read)
    bases = torch.empty(n_rec * read, dtype=torch.uint8, device="cuda")
    L.smh_synth_dna_dev(C.c_void_p(bases.data_ptr()), 0, bases.numel(), 4, 0, C.c_void_p(0))
    torch.cuda.synchronize()
    rec = 12 + (read + 1) + 2 + (read + 1)
    text = torch.empty((n_rec, rec), dtype=torch.uint8, device="cuda")
    idx = torch.arange(n_rec, device="cuda", dtype=torch.int64)
    text[:, 0] = 0x40
    for d in range(10):
        text[:, 10 - d] = ((idx // 10 ** d) % 10 + 48).to(torch.uint8)
    text[:, 11] = 0x0A
    text[:, 12:12 + read] = bases.view(n_rec, read)
    text[:, 12 + read] = 0x0A
    text[:, 13 + read] = 0x2B
    text[:, 14 + read] = 0x0A
    text[:, 15 + read:15 + 2 * read] = 0x49
    text[:, 15 + read] = 0x40
    text[:, 15 + 2 * read] = 0x0A
    del idx
    off = np.arange(n_rec + 1, dtype=np.uint64) * np.uint64(read)
    return text.view(-1), bases, off


def prof(L, name):
    ms, cnt = C.c_double(), C.c_uint64()
    L.smh_profile_get(name, C.byref(ms), C.byref(cnt))
    return ms.value, cnt.value


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def measure(args):
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    L = pkg.lib()
    n_bases = int(args.gb * 1e9)
    mx = (1 << 64) // 1000
    result = {"gb_of_bases": args.gb, "runs": RUNS, "copy_rate_bytes_per_s": COPY_RATE, "inputs": {}}
    for fmt, make in (("fasta", fasta_on_device), ("fastq", fastq_on_device)):
        text, bases, off = make(torch, L, n_bases)
        nrec, kept, nbytes = off.size - 1, int(off[-1]), text.numel()
        new = lambda: pkg.KmerMinHash(0, 31, False, 42, mx, True)   # noqa: E731

        def parse_only():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = pkg.Records.parse(text, fmt)
            return time.perf_counter() - t0, r

        def parse_and_sketch():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            mh = new()
            mh.add_records(pkg.Records.parse(text, fmt), True)
            return time.perf_counter() - t0, mh

        def sketch_cut():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            mh = new()
            mh.add_sequences_dev(bases.data_ptr(), kept, off, True)
            return time.perf_counter() - t0, mh

        _, r = parse_only()                                          # warm-up, and the checks
        assert len(r) == nrec and r.total == kept
        assert np.array_equal(r.offsets, off)
        got = r.seq_tensor()
        assert torch.equal(got[:1 << 20], bases[:1 << 20]) and torch.equal(got[-(1 << 20):], bases[-(1 << 20):])
        del got, r
        _, a = parse_and_sketch()
        _, b = sketch_cut()
        assert np.array_equal(a.mins_np(), b.mins_np()) and np.array_equal(a.abunds_np(), b.abunds_np())
        if args.trace_child:
            continue
        L.smh_profile_reset(); L.smh_profile_enable(1)
        t_parse, t_both, t_cut = [], [], []
        for _ in range(RUNS):                                        # alternating
            t_parse.append(parse_only()[0])
            t_both.append(parse_and_sketch()[0])
            t_cut.append(sketch_cut()[0])
        scan_ms, n1 = prof(L, b"parse_scan")
        comp_ms, n2 = prof(L, b"parse_compact")
        L.smh_profile_enable(0)
        floor = (2 * nbytes + kept) / COPY_RATE
        kernels = (scan_ms / n1 + comp_ms / n2) / 1e3
        result["inputs"][fmt] = {
            "records": nrec, "text_bytes": nbytes, "kept_bytes": kept,
            "parse_call_s": spread(t_parse), "parse_text_gb_per_s": nbytes / statistics.median(t_parse) / 1e9,
            "parse_kernels_s": kernels, "parse_kernels_text_gb_per_s": nbytes / kernels / 1e9,
            "summary_and_scan_ms": scan_ms / n1, "compact_ms": comp_ms / n2,
            "floor_s": floor, "share_of_floor_kernels": floor / kernels, "share_of_floor_call": floor / statistics.median(t_parse),
            "parse_plus_add_records_s": spread(t_both), "add_sequences_dev_on_cut_records_s": spread(t_cut),
            "ratio_parse_plus_sketch_over_cut": spread([x / y for x, y in zip(t_both, t_cut)]),
        }
        del text, bases, a, b
        torch.cuda.empty_cache()
        L.smh_release_workspace()
    if not args.trace_child:
        # (c) the offsets of 28 M records read back on their own: 150-base reads, the whole parse call beside it
        text, bases, off = fastq_on_device(torch, L, 28_000_000 * 150)
        pkg.Records.parse(text, "fastq")
        whole = []
        for _ in range(RUNS):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = pkg.Records.parse(text, "fastq")
            whole.append(time.perf_counter() - t0)
        dev_off = torch.from_numpy(off.view(np.int64)).cuda()
        pinned = torch.empty(off.size, dtype=torch.int64).pin_memory()
        back = []
        for _ in range(RUNS + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            pinned.copy_(dev_off); torch.cuda.synchronize()
            back.append(time.perf_counter() - t0)
        result["offsets_readback_28M"] = {"bytes": int(off.size * 8), "copy_s": spread(back[1:]), "parse_call_s": spread(whole)}
    print("BENCH_FASTX " + json.dumps(result))


def kernel_stats(directory):
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"k_(parse_\w+|scan_\w+|first_content)", row["Name"])
                if m:
                    name = m.group(0) + ("_fasta" if "FastaScan" in row["Name"] else "_fastq" if "FastqScan" in row["Name"] else "")
                    out[name] = {"calls": int(row["Calls"]), "total_ms": int(row["TotalDurationNs"]) / 1e6,
                                 "average_ms": float(row["AverageNs"]) / 1e6}
    return out


def child(extra, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + extra
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=280)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        raise SystemExit("child failed: %s (exit %d)" % (" ".join(cmd), p.returncode))
    return p.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_bench_fastx.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--measure-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.measure_child or args.trace_child:
        return measure(args)
    out = child(["--measure-child", "--gb", str(args.gb)])
    line = [ln for ln in out.splitlines() if ln.startswith("BENCH_FASTX ")][-1]
    result = json.loads(line[len("BENCH_FASTX "):])
    if not args.no_trace:
        # the warm-up calls of a run of its own under the tracer: two parses and one sketch per format
        with tempfile.TemporaryDirectory() as d:
            child(["--trace-child", "--gb", str(args.gb)],
                  prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"])
            result["kernel_trace"] = kernel_stats(d)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
