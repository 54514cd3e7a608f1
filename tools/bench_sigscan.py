"""Signature JSON read on the device on one GPU: writes profiles/r24_bench_sigscan.json.

    python tools/bench_sigscan.py [--host-seconds 60] [--max-sketches 200000] [--out profiles/r24_bench_sigscan.json]

Input: a database from synth.family_signatures (bottom-2000 sketches, k = 31), serialised by save_signatures in documents of 500
signatures.  Its size is chosen from a timed sample so that the host route takes about --host-seconds, but at most
--max-sketches: the text and both routes' sketches are held in host memory at once, 40 KB of text per sketch (200 000 sketches
are 8 GB of text, which the host route reads in 15 to 18 s).  The size and whether the cap cut it are recorded.
Whole calls, medians of 3, in turns, after both routes were asserted to give equal read() and equal entries:
(a) SignatureScan.parse(text, doc_offsets) + ResidentIndex.from_signatures: the text is uploaded once and read on the device;
(b) the parent commit's route: load_signatures_buffer per document + ResidentIndex(sketches);
(c) a plain upload of the text: the link floor.
Also: the parse alone from host text, and parse and index alone (C calls) on a text already in HBM.
Kernel time by HIP events (sigscan_summary, sigscan_scan, sigscan_compact; the gather's copy and checks) on a text already in
HBM, as GB/s of text and as a share of the traffic floor (the text read twice, 8 B per token and the skeleton written) /
6.3 TB/s."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.3e12          # bytes / s, measured streaming rate of the part
RUNS = 3
PER_DOC = 500
NUM = 2000


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def prof(L, name):
    ms, cnt = C.c_double(), C.c_uint64()
    L.smh_profile_get(name, C.byref(ms), C.byref(cnt))
    return ms.value, cnt.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-seconds", type=float, default=60.0, help="what the host route should take on the input (default 60)")
    ap.add_argument("--max-sketches", type=int, default=200000,
                    help="cap on the input's size: 40 KB of text per sketch, held in host memory next to both routes' sketches "
                         "(default 200000 = 8 GB of text, 15 to 18 s on the host route)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_bench_sigscan.json"))
    args = ap.parse_args()
    import warnings
    import numpy as np
    import torch
    warnings.filterwarnings("ignore", message=".*not writable.*")    # (the uploads read host bytes in place)
    from __graft_entry__ import load_package
    pkg = load_package()
    from sourmash_rust_amd import signature as sg, synth
    L = pkg.lib()

    def documents(lo, hi):
        docs = []
        for a in range(lo, hi, PER_DOC):
            rows = synth.family_signatures(a, min(a + PER_DOC, hi), num=NUM)
            sigs = []
            for i, row in enumerate(rows):
                mh = pkg.KmerMinHash(NUM, 31)
                mh.add_many(row)
                s = sg.Signature()
                s.name = "synthetic %d" % (a + i)
                s.push_mh(mh)
                sigs.append(s)
            docs.append(sg.save_signatures(sigs).encode())
        return docs

    def host_route(docs):
        sigs = [s for d in docs for s in sg.load_signatures_buffer(d)]
        return sigs, pkg.index.ResidentIndex([s.first_mh() for s in sigs])

    def device_route(text, offs):
        scan = sg.SignatureScan.parse(text, offs)
        return scan, pkg.index.ResidentIndex.from_signatures(scan)

    def offsets(docs):
        return np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    sample = documents(0, 2 * PER_DOC)
    host_route(sample[:1]); device_route(sample[0], offsets(sample[:1]))                  # warm-up
    t_sample = timed(lambda: host_route(sample))[0]
    wanted = 2 * PER_DOC * args.host_seconds / t_sample
    n = int(max(2 * PER_DOC, min(args.max_sketches, wanted)) // PER_DOC * PER_DOC)
    print("sample: %d sketches in %.2f s on the host route -> %d sketches (%d for %.0f s)" % (2 * PER_DOC, t_sample, n, wanted, args.host_seconds),
          flush=True)
    docs = sample + documents(2 * PER_DOC, n)
    offs = offsets(docs)
    text = b"".join(docs)

    (sigs, host), (scan, dev) = host_route(docs), device_route(text, offs)
    for x, y in zip(host.read(), dev.read()):
        assert (x is None and y is None) or np.array_equal(x, y)
    assert [(e.name, e.num, e.ksize, e.seed, e.max_hash, e.molecule, e.n_mins) for e in scan.entries] == \
        [(s.name, m.num, m.ksize, m.seed, m.max_hash, m.molecule, len(m)) for s in sigs for m in [s.first_mh()]]
    spans = scan.spans()
    skeleton = len(text) - sum(s["end"] - s["start"] for s in spans)
    tokens = scan.n_tokens
    del sigs, host, dev, scan

    def upload():
        return torch.from_numpy(np.frombuffer(text, dtype=np.uint8)).cuda()

    routes = {"a_device": lambda: device_route(text, offs), "b_host_loader": lambda: host_route(docs), "c_upload_text": upload,
              "a1_parse_alone": lambda: sg.SignatureScan.parse(text, offs)}
    times = {k: [] for k in routes}
    for _ in range(RUNS):                                            # in turns
        for name, fn in routes.items():
            times[name].append(timed(fn)[0])
        print({k: round(v[-1], 3) for k, v in times.items()}, flush=True)

    text_dev = upload()
    in_hbm = {"parse_dev": [], "index": []}
    L.smh_profile_reset(); L.smh_profile_enable(1)
    for _ in range(RUNS):
        t, scan = timed(lambda: sg.SignatureScan.parse(text_dev, offs))
        in_hbm["parse_dev"].append(t)
        in_hbm["index"].append(timed(lambda: L.smh_index_free(L.smh_signatures_index(scan._p, None, 0)))[0])
    kernels = {}
    for name in (b"sigscan_summary", b"sigscan_scan", b"sigscan_compact", b"sigscan_gather", b"downsample_copy"):
        ms, cnt = prof(L, name)
        kernels[name.decode()] = {"ms": ms / max(cnt, 1) * (cnt / RUNS), "launches_per_call": cnt / RUNS}
    L.smh_profile_enable(0)
    scan_ms = sum(kernels[k]["ms"] for k in ("sigscan_summary", "sigscan_scan", "sigscan_compact"))
    floor_s = (2 * len(text) + 8 * tokens + skeleton) / COPY_RATE
    med = {k: statistics.median(v) for k, v in times.items()}
    result = {
        "sketches": n, "sketches_for_host_seconds": int(wanted), "host_seconds_wanted": args.host_seconds,
        "capped_by_max_sketches": wanted > args.max_sketches, "hashes_per_sketch": NUM, "documents": len(docs), "text_bytes": len(text), "skeleton_bytes": skeleton,
        "tokens": tokens, "spans": len(spans), "runs": RUNS, "copy_rate_bytes_per_s": COPY_RATE,
        "calls_s": {k: spread(v) for k, v in times.items()}, "text_gb_per_s": {k: len(text) / v / 1e9 for k, v in med.items()},
        "b_over_a": med["b_host_loader"] / med["a_device"], "a_over_c": med["a_device"] / med["c_upload_text"],
        "kernels_ms": kernels, "text_in_hbm_calls_s": {k: spread(v) for k, v in in_hbm.items()},
        "scan_kernels": {"ms": scan_ms, "text_gb_per_s": len(text) / (scan_ms / 1e3) / 1e9, "floor_ms": floor_s * 1e3,
                         "share_of_floor": floor_s / (scan_ms / 1e3)},
    }
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
