"""Zip collections loaded on the device on one GPU: writes profiles/r26_bench_archive.json.

    python tools/bench_archive.py [--sketches 8000] [--out profiles/r26_bench_archive.json]

Input: the synth.family_signatures collection of tools/bench_sigscan.py (bottom-2000 sketches, k = 31, about 40 KB of .sig text
each), one signature per member, as a zip of stored `signatures/<i>.sig.gz` members (gzip level 6, mtime 0) with a
SOURMASH-MANIFEST.csv.  Conditions: one run, medians of 3 whole calls taken in turns, equal read() asserted first.
Routes: (a) ResidentIndex.from_zip; (b) zipfile + gzip.decompress per member on 16 threads, then SignatureScan.parse +
from_signatures -- the best the library could do before; (c) the upload of the compressed file alone.  Then the kernels by HIP
events against their traffic floor; the same collection with one member of 2 MB of text added, handed out longest first and in
id order (smh_archive_set_sorted); and a lone member of 64 KiB ... 16 MiB of text, the device against one-thread zlib + upload,
from which the default device_member_limit follows: the largest power of two at which the device takes at most twice the host's
time (on the device the member overlaps with all the others, on the host it holds up the call)."""
import argparse
import concurrent.futures
import csv
import ctypes as C
import gzip
import io
import json
import os
import statistics
import sys
import time
import zipfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.3e12          # bytes / s, measured streaming rate of the part
RUNS = 3
NUM = 2000
THREADS = 16


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def prof(L, name):
    ms, cnt = C.c_double(), C.c_uint64()
    L.smh_profile_get(name, C.byref(ms), C.byref(cnt))
    return ms.value, cnt.value


def sig_text(name, mins):
    return ('[{"class":"sourmash_signature","email":"","hash_function":"0.murmur64","filename":null,"name":"%s","license":"CC0",'
            '"signatures":[{"num":%d,"ksize":31,"seed":42,"max_hash":0,"mins":[%s],"md5sum":"%032x","molecule":"DNA"}],"version":0.4}]'
            % (name, len(mins), ",".join(map(str, mins)), zlib.crc32(name.encode()))).encode()


def make_zip(texts, names):
    with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
        members = list(pool.map(lambda t: gzip.compress(t, 6, mtime=0), texts))
    buf = io.BytesIO()
    rows = io.StringIO()
    rows.write("# SOURMASH-MANIFEST-VERSION: 1.0\n")
    w = csv.writer(rows)
    w.writerow(["internal_location", "md5", "md5short", "ksize", "moltype", "num", "scaled", "n_hashes", "with_abundance", "name", "filename"])
    with zipfile.ZipFile(buf, "w") as z:
        for i, (m, name) in enumerate(zip(members, names)):
            loc = "signatures/%d.sig.gz" % i
            z.writestr(zipfile.ZipInfo(loc), m, compress_type=zipfile.ZIP_STORED)
            w.writerow([loc, "%032x" % i, "%08x" % i, 31, "DNA", NUM, 0, NUM, 0, name, ""])
        z.writestr(zipfile.ZipInfo("SOURMASH-MANIFEST.csv"), rows.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=8000, help="members of the collection (default 8000 = 0.3 GB of text)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_bench_archive.json"))
    args = ap.parse_args()
    import warnings
    import numpy as np
    import torch
    warnings.filterwarnings("ignore", message=".*not writable.*")
    from __graft_entry__ import load_package
    pkg = load_package()
    from sourmash_rust_amd import archive, signature as sg, synth
    L = pkg.lib()
    RI = pkg.index.ResidentIndex

    n = args.sketches
    rows = synth.family_signatures(0, n, num=NUM)
    names = ["synthetic %d" % i for i in range(n)]
    texts = [sig_text(names[i], rows[i].tolist()) for i in range(n)]
    data = make_zip(texts, names)
    text_bytes = sum(len(t) for t in texts)
    print("collection: %d members, %.1f MB of text, %.1f MB compressed" % (n, text_bytes / 1e6, len(data) / 1e6), flush=True)

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def host_members(blob):
        with zipfile.ZipFile(io.BytesIO(blob)) as z:
            infos = [i for i in z.infolist() if i.filename.endswith(".sig.gz")]
            raws = [z.read(i) for i in infos]
        with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
            return list(pool.map(gzip.decompress, raws))

    def route_b(blob):
        docs = host_members(blob)
        offs = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
        return RI.from_signatures(sg.SignatureScan.parse(b"".join(docs), offs))

    def upload(blob):
        return torch.from_numpy(np.frombuffer(blob, dtype=np.uint8)).cuda()

    a, b = RI.from_zip(data), route_b(data)                      # warm-up, and the equality every figure rests on
    for x, y in zip(a.read(), b.read()):
        assert (x is None and y is None) or np.array_equal(x, y)
    assert [e.name for e in a.signatures] == names
    del a, b
    routes = {"a_from_zip": lambda: RI.from_zip(data), "b_zipfile_gzip_16_threads_parse": lambda: route_b(data), "c_upload_compressed": lambda: upload(data)}
    times = {k: [] for k in routes}
    for _ in range(RUNS):                                        # in turns
        for k, fn in routes.items():
            t, out = timed(fn)
            times[k].append(t)
            del out
    result = {"sketches": n, "text_bytes": text_bytes, "compressed_bytes": len(data), "runs": RUNS,
              "routes_s": {k: spread(v) for k, v in times.items()}}
    print(json.dumps(result["routes_s"]), flush=True)

    # the kernels by HIP events
    zc = archive.ZipCollection(data)
    ids = zc.select()
    L.smh_profile_enable(1)
    kern = {}
    for verify in (True, False):
        per = {k: [] for k in ("archive_inflate", "archive_chunks", "archive_crc")}
        for _ in range(RUNS):
            L.smh_profile_reset()
            zc.text(ids, verify=verify)
            for k in per:
                per[k].append(prof(L, k.encode())[0])
        kern["verify" if verify else "no_verify"] = {k: spread(v) for k, v in per.items()}
    L.smh_profile_enable(0)
    floor_ms = (len(data) + 2 * text_bytes) / COPY_RATE * 1e3    # compressed read, text written, text read for the CRC
    total_ms = sum(v["median"] for v in kern["verify"].values())
    result["kernels_ms"] = kern
    result["traffic_floor_ms"] = floor_ms
    result["kernels_share_of_floor"] = floor_ms / total_ms if total_ms else None
    result["text_call_s"] = spread([timed(lambda: zc.text(ids))[0] for _ in range(RUNS)])
    print(json.dumps(kern), flush=True)

    # one long member among the small ones: what the queue is for
    big = sig_text("big", list(range(10 ** 18, 10 ** 18 + 100000)))
    assert 1.9e6 < len(big) < 2.3e6
    zc_big = archive.ZipCollection(make_zip(texts + [big], names + ["big"]))
    ids_big = zc_big.select()
    assert zc_big.entries[ids_big[-1]].text_size == len(big)
    order = {}
    for label, flag in (("longest_first", 1), ("id_order", 0), ("longest_first_again", 1)):
        L.smh_archive_set_sorted(flag)
        order[label] = spread([timed(lambda: zc_big.text(ids_big, device_member_limit=1 << 30))[0] for _ in range(RUNS)])
    L.smh_archive_set_sorted(1)
    result["one_2mb_member_added_text_call_s"] = order
    print(json.dumps(order), flush=True)

    # a lone member: the device against one-thread zlib + upload
    sweep, limit = [], None
    for shift in range(16, 25):
        size = 1 << shift
        body = sig_text("lone", list(range(10 ** 18, 10 ** 18 + size // 20)))[:size]
        lone = make_zip([body], ["lone"])
        z1 = archive.ZipCollection(lone)
        member = lone[z1.entries[0].data_off:z1.entries[0].data_off + z1.entries[0].comp_size]
        z1.text([0], device_member_limit=1 << 30)
        dev = spread([timed(lambda: z1.text([0], device_member_limit=1 << 30))[0] for _ in range(RUNS)])
        hst = spread([timed(lambda: upload(gzip.decompress(member)))[0] for _ in range(RUNS)])
        sweep.append({"text_bytes": size, "device_s": dev, "host_zlib_upload_s": hst})
        if dev["median"] <= 2 * hst["median"]:
            limit = size
    result["lone_member_sweep"] = sweep
    result["device_member_limit_rule"] = "largest power of two of the sweep at which device <= 2 x (one-thread zlib + upload)"
    result["device_member_limit_measured"] = limit
    result["device_member_limit_default"] = archive.DEFAULT_DEVICE_MEMBER_LIMIT
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
