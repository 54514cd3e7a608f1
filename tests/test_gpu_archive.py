"""Zip collections inflated on the device (archive.ZipCollection, ResidentIndex.from_zip, C ABI smh_archive_*; DESIGN.md
3.29): the text byte for byte against zipfile + gzip, statuses against tests/archive_restatement.py -- whose crafted archives
the host build of the same source has passed under the sanitizers (tests/test_archive_host.py) -- every chunk count, block
kind and copy shape, member mixes under grid caps and the pool fill, a text past 4 GiB, the way through the parser to a
resident index, and stream order.  C is the CRC chunk (smh_archive_geometry)."""
import csv
import ctypes as C
import glob
import gzip
import io
import json
import os
import random
import struct
import zipfile
import zlib

import numpy as np
import pytest

import archive_restatement as R
import inflate_restatement as IR
import sigscan_restatement as SR
import stream_order as SO
from conftest import GOLDEN

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

u32p, u64p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def ar(pkg):
    from sourmash_rust_amd import archive
    chunk, threads = C.c_uint32(), C.c_uint32()
    pkg.lib().smh_archive_geometry(C.byref(chunk), C.byref(threads))
    assert chunk.value == R.CHUNK and threads.value % 64 == 0
    return archive


def host(t):
    return bytes(t.cpu().numpy())


def by_zipfile(data):
    """{name: text} as zipfile and gzip give it"""
    out = {}
    with zipfile.ZipFile(io.BytesIO(data)) as z:
        for info in z.infolist():
            content = z.read(info)
            out[info.filename] = gzip.decompress(content) if content[:2] == b"\x1f\x8b" else content
    return out


def device(pkg, ar, data, ids=None, offs=None, verify=True, stream=None, comp=None, cap=None):
    """one smh_archive_inflate_dev call: (zc, text bytes with the sentinel tail cut off, statuses, error message or None).
    The output has 64 sentinel bytes behind the text, which must survive."""
    zc = data if isinstance(data, ar.ZipCollection) else ar.ZipCollection(data)
    ids = list(range(len(zc))) if ids is None else list(ids)
    sizes = [zc.entries[i].text_size if i < len(zc) else 0 for i in ids]
    if offs is None:
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)[:len(ids)] if ids else np.zeros(0, np.uint64)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    total = int(max([int(o) + s for o, s in zip(offs, sizes)], default=0)) if cap is None else cap
    out = torch.full((total + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    if comp is None:
        comp = torch.frombuffer(bytearray(zc.data), dtype=torch.uint8).cuda()
    status = np.full(max(len(ids), 1), 0xEE, dtype=np.uint8)
    v = np.array(ids, dtype=np.uint32)
    torch.cuda.synchronize()
    code = pkg.lib().smh_archive_inflate_dev(zc._p, C.c_void_p(comp.data_ptr()), len(zc.data), v.ctypes.data_as(u32p), offs.ctypes.data_as(u64p),
                                             len(ids), C.c_void_p(out.data_ptr()), total, int(verify), status.ctypes.data_as(u8p),
                                             C.c_void_p(stream or 0))
    err = None
    if code:
        assert code == 3
        err = _last_message(pkg)
    assert bool((out[total:] == SENTINEL).all()), "bytes behind the text were written"
    return zc, out[:total], status[:len(ids)], err


def _last_message(pkg):
    from sourmash_rust_amd.errors import take_str
    L = pkg.lib()
    msg = take_str(L.sourmash_err_get_last_message()).decode()
    L.sourmash_err_clear()
    return msg


pattern = R.pattern                                              # a text with literals, near and far matches


def check_valid(pkg, ar, data, **kw):
    want = by_zipfile(data)
    zc, out, status, err = device(pkg, ar, data, **kw)
    assert err is None and not status.any(), (err, status.nonzero())
    text, at = host(out), 0
    for e in zc.entries:
        assert text[at:at + e.text_size] == want[e.name], e.name
        at += e.text_size
    assert at == len(text)
    return zc


# ------------------------------------------------------------------------------------------------------ sizes, kinds, levels
def test_every_chunk_count_as_every_kind(pkg, ar):
    Ck = R.CHUNK
    sizes = (0, 1, Ck - 1, Ck, Ck + 1, 2 * Ck + 1, 65 * Ck + 1, 65536, 65537, (1 << 20) + 1)
    members = []
    for k, size in enumerate(sizes):
        t = pattern(size, k)
        members += [R.member("d%d.sig" % size, t, 8), R.member("s%d.sig" % size, t), R.member("g%d.sig.gz" % size, R.gz(t))]
    data = R.build(members)
    for verify in (True, False):
        zc = check_valid(pkg, ar, data, verify=verify)
    assert [e.kind for e in zc.entries[3:6]] == ["deflate", "stored", "gzip"]
    assert [(e.kind, e.text_size) for e in zc.entries[:3]] == [("deflate", 0), ("stored", 0), ("gzip", 0)]
    assert max(R.chunks_of(e.text_size) for e in zc.entries) > 64                     # more chunks than lanes in the fold


def test_levels_and_strategies(pkg, ar):
    members = []
    for size in (2 * R.CHUNK + 1, 65537):
        t = pattern(size, size)
        for level in (0, 1, 6, 9):
            members.append(R.member("l%d_%d.sig" % (level, size), t, 8, level=level))
            members.append(R.member("l%d_%d.sig.gz" % (level, size), R.gz(t, level)))
        for name, strategy in (("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
            members.append(R.member("%s_%d.sig" % (name, size), t, 8, strategy=strategy))
            members.append(R.member("%s_%d.sig.gz" % (name, size), R.gz(t, 6, strategy)))
    members.append(R.member("fibonacci.sig", IR.fibonacci_text(), 8, strategy=zlib.Z_HUFFMAN_ONLY))
    data = R.build(members)
    stored_blocks = R.raw_deflate(pattern(65537, 65537), 0)
    assert stored_blocks[0] & 6 == 0 and len(stored_blocks) > 65537                   # level 0: stored blocks, two of them
    check_valid(pkg, ar, data)


def far_match_member():
    """a stream zlib never writes: matches at distance 32 768 (zlib stops 262 short of it) that lie across the 64 KiB line,
    behind a stored block of 65 000 bytes"""
    rng = random.Random(77)
    first = bytes(rng.randrange(256) for _ in range(65000))
    text = bytearray(first)
    w = IR.BitWriter().put(1, 1).put(1, 2)
    for length, dist in ((258, 32768), (258, 32768), (300 - 258 + 216, 32768), (3, 32768), (258, 1), (100, 32767), (258, 32768)):
        w.fixed_match(length, dist)
        for _ in range(length):
            text.append(text[-dist])
    payload = b"\x00" + struct.pack("<HH", 65000, 65000 ^ 0xFFFF) + first + w.fixed_lit(256).bytes()
    assert len(text) > 65536 + 600 and zlib.decompress(payload, -15) == bytes(text)
    return payload, bytes(text)


def test_matches_at_distance_32768_across_the_64_kib_line(pkg, ar):
    payload, text = far_match_member()
    trailer = struct.pack("<II", zlib.crc32(text), len(text))
    data = R.build([R.member("far.sig", text, 8, comp=payload), R.member("far.sig.gz", b"\x1f\x8b\x08\x00\0\0\0\0\x00\xff" + payload + trailer)])
    check_valid(pkg, ar, data)


def test_every_output_and_payload_phase(pkg, ar):
    rng = random.Random(3)
    members = []
    for i in range(64):
        t = bytes(rng.choice(b"ACGT\n") for _ in range(2 * (i % 5) + 1 + 16 * (i % 3)))
        name = "m%02d%s.sig" % (i, "x" * (i % 4))                # names of four lengths: the data starts at every phase mod 4
        members.append(R.member(name, t, (8, 0)[i % 2]) if i % 3 else R.member(name + ".gz", R.gz(t, name=b"n" * (i % 4))))
    data = R.build(members)
    zc = ar.ZipCollection(data)
    assert {e.payload_off % 4 for e in zc.entries if e.kind != "stored"} == set(range(4))
    assert {e.payload_off % 4 for e in zc.entries if e.kind == "stored"} == set(range(4))
    want = by_zipfile(data)
    offs, at = [], 0
    for k, e in enumerate(zc.entries):                           # slices apart from each other, at every phase mod 16
        at += (k % 16 - at) % 16
        offs.append(at)
        at += e.text_size
    assert {o % 16 for o in offs} == set(range(16))
    _, out, status, err = device(pkg, ar, zc, offs=offs)
    assert err is None and not status.any()
    text = host(out)
    for e, o in zip(zc.entries, offs):
        assert text[o:o + e.text_size] == want[e.name]
    gaps = bytearray(text)
    for e, o in zip(zc.entries, offs):
        gaps[o:o + e.text_size] = bytes([SENTINEL]) * e.text_size
    assert bytes(gaps) == bytes([SENTINEL]) * len(text)          # nothing between the slices was written
    lead = torch.frombuffer(bytearray(b"\xff" * 3 + data), dtype=torch.uint8).cuda()[3:]          # the file at an odd address
    _, out2, status, err = device(pkg, ar, zc, offs=offs, comp=lead)
    assert err is None and host(out2) == text


# ------------------------------------------------------------------------------------------------ member mixes and the queue
@pytest.fixture(scope="module")
def mix():
    """300 members of mixed kinds and sizes, two long ones late in the archive: `order` is far from the identity"""
    members = []
    for i in range(300):
        size = (3 * R.CHUNK + 5) if i == 251 else (100000 + i) if i == 299 else (i * 37) % 3000
        t = pattern(size, 1000 + i)
        kind = i % 4
        if kind == 0:
            members.append(R.member("signatures/%d.sig.gz" % i, R.gz(t)))
        elif kind == 1:
            members.append(R.member("signatures/%d.sig" % i, t, 8, strategy=(zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY)[i % 3]))
        elif kind == 2:
            members.append(R.member("signatures/%d.sig" % i, t))
        else:
            members.append(R.member("signatures/%d.sig.gz" % i, R.gz(t, 1)))
    return members


@pytest.mark.parametrize("fill", [-1, 0xA5])
@pytest.mark.parametrize("cap", [0, 1, 3])
def test_member_mixes_under_grid_caps_and_pool_fill(pkg, ar, mix, cap, fill):
    L = pkg.lib()
    L.smh_set_grid_cap(cap)
    L.smh_set_pool_fill(fill)
    try:
        for n in (1, 2, 64, 65, 300):
            data = R.build(mix[300 - n:])
            zc = check_valid(pkg, ar, data)
            lens = [e.payload_len for e in zc.entries if e.kind != "stored"]
            assert n < 64 or lens != sorted(lens, reverse=True)
    finally:
        L.smh_set_grid_cap(0)
        L.smh_set_pool_fill(-1)


def test_the_identity_order_gives_the_same_text(pkg, ar, mix):
    L = pkg.lib()
    data = R.build(mix)
    L.smh_archive_set_sorted(0)
    try:
        check_valid(pkg, ar, data)
    finally:
        L.smh_archive_set_sorted(1)


def test_ids_reversed_repeated_and_a_subset(pkg, ar, mix):
    data = R.build(mix[200:])
    zc = ar.ZipCollection(data)
    want = by_zipfile(data)
    n = len(zc)
    for ids in (list(range(n))[::-1], [99, 99, 51, 99, 0, 51], list(range(3, n, 7)), []):
        _, out, status, err = device(pkg, ar, zc, ids=ids)
        assert err is None and not status.any()
        assert host(out) == b"".join(want[zc.entries[i].name] for i in ids)


def test_past_4_gib(pkg, ar):
    t = pattern(65536, 5)
    tail = pattern(777, 6)
    data = R.build([R.member("one.sig.gz", R.gz(t)), R.member("tail.sig", tail, 8)])
    n = 70000
    ids = [0] * n + [1]
    zc, out, status, err = device(pkg, ar, data, ids=ids)
    assert err is None and not status.any() and out.numel() == n * 65536 + 777 > 1 << 32
    ref = torch.frombuffer(bytearray(t), dtype=torch.uint8).cuda()
    for lo in range(0, n, 10000):                                # (in slabs: the comparison's temporary stays small)
        assert bool((out[lo * 65536:(lo + 10000) * 65536].view(-1, 65536) == ref).all())
    assert host(out[n * 65536:]) == tail
    del out


# ------------------------------------------------------------------------------------------------------------ bad members
BAD = {"flipped_payload": None, "wrong_crc": [IR.CRC, IR.CRC], "wrong_trailer": [IR.CRC], "gzip_two_members": [IR.LEFTOVER],
       "bad_mix": None, "host_served": None, "trailer_and_good": [IR.CRC, IR.OK], "equal_halves": [IR.LEFTOVER],
       "reserved_block": [IR.BLOCK_TYPE, IR.OK]}


@pytest.mark.parametrize("name", sorted(BAD))
def test_statuses_equal_the_restatements(pkg, ar, name):
    data = dict(R.crafted())[name]                               # (the host build has passed exactly these bytes)
    entries = R.scan(data)
    for verify in (True, False):
        want = [R.status(data, e, verify)[1] for e in entries]
        assert BAD[name] is None or not verify or want == BAD[name]
        zc, out, status, err = device(pkg, ar, data, verify=verify)
        assert status.tolist() == want, (name, verify)
        if any(want):
            low = next(i for i, w in enumerate(want) if w)
            assert err is not None and err.startswith("archive: ") and "(entry %d '%s')" % (low, zc.entries[low].name) in err, err
        else:
            assert err is None


def test_good_members_next_to_bad_ones_are_right(pkg, ar):
    data, good = R.bad_mix()
    assert data == dict(R.crafted())["bad_mix"]                  # (the host build has passed exactly these bytes)
    entries = R.scan(data)
    want = [R.status(data, e)[1] for e in entries]
    assert want[::2] == [0] * 6 and all(want[1::2]) and want[7] == IR.OUT_OVER
    zc, out, status, err = device(pkg, ar, data)
    assert status.tolist() == want and "(entry 1 'bad_crc.sig')" in err and "CRC" in err
    text, at = host(out), 0
    for k, e in enumerate(zc.entries):
        if k % 2 == 0:
            assert text[at:at + e.text_size] == good[k // 2]
        at += e.text_size


def test_arguments_are_refused_before_anything_is_launched(pkg, ar):
    data = R.build([R.member("a.sig", pattern(100, 1), 8), R.member("b.sig", pattern(50, 2)), R.member("e.sig", b"x", flags=1)])
    zc = ar.ZipCollection(data)
    for kw, words in ((dict(ids=[0, 1], offs=[0, 99]), "overlap"), (dict(ids=[0, 1], offs=[0, 100], cap=149), "leaves the output"),
                      (dict(ids=[0, 2], offs=[0, 100]), "encrypted entry"), (dict(ids=[0, 3], offs=[0, 100]), "entry 3 of 3"),
                      (dict(ids=[1, 0, 1], offs=[0, 60, 20]), "overlap")):
        _, out, status, err = device(pkg, ar, zc, **kw)
        assert err is not None and words in err, (kw, err)
        assert bool((out == SENTINEL).all()) and set(status.tolist()) == {0xEE}
    L = pkg.lib()
    comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    ids, offs = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    out = torch.zeros(100, dtype=torch.uint8, device="cuda")
    assert L.smh_archive_inflate_dev(zc._p, C.c_void_p(comp.data_ptr()), len(data) - 1, ids.ctypes.data_as(u32p), offs.ctypes.data_as(u64p), 1,
                                     C.c_void_p(out.data_ptr()), 100, 1, None, None) == 3
    assert not out.any()


# -------------------------------------------------------------------------------------------------------- the Python layer
def test_text_serves_what_the_device_does_not_take_from_the_host(pkg, ar):
    crafted = dict(R.crafted())                                  # (every archive here has passed the host build first)
    data, (a, b, c, d) = R.host_served()
    assert data == crafted["host_served"]
    zc = ar.ZipCollection(data)
    assert zc.manifest is None and zc.select() == [0, 1, 2, 3, 4] and zc.select(names=["c.sig", "plain.sig"]) == [2, 4]
    assert [e.kind for e in zc.entries] == ["gzip", "gzip", "deflate", "deflate", "stored", "stored"]
    # in C the two-member .gz is refused: its first member ends below the ISIZE of the last
    entries = R.scan(data)
    want = [R.status(data, entries[i])[1] for i in (0, 1)]
    assert want == [IR.OUT_UNDER, IR.OK]
    _, _, status, err = device(pkg, ar, zc, ids=[0, 1])
    assert status.tolist() == want and "(entry 0 'two.sig.gz')" in err
    for limit in (None, 1 << 30, len(c) - 1, 0):
        status = np.full(5, 0xEE, dtype=np.uint8)
        text, offs = zc.text(device_member_limit=limit, status=status)
        assert host(text) == a + b + c + d + a and offs.tolist() == np.cumsum([0] + [len(x) for x in (a, b, c, d, a)]).tolist()
        assert not status.any()
    text, offs = zc.text([4, 1, 1])
    assert host(text) == a + b + b and offs.tolist() == [0, len(a), len(a) + len(b), len(a) + 2 * len(b)]
    text, offs = zc.text([])
    assert text.numel() == 0 and offs.tolist() == [0]
    # a member that is really bad stays an error: the host is asked only for what gzip can explain
    bad, (b2, c2) = R.trailer_and_good()
    assert bad == crafted["trailer_and_good"]
    with pytest.raises(pkg.SourmashError) as err:
        ar.ZipCollection(bad).text()
    assert err.value.code == 3 and "CRC" in err.value.message and "(entry 0 'bad.sig.gz')" in err.value.message
    assert host(ar.ZipCollection(bad).text(verify=False)[0]) == b2 + c2
    # a deflate entry zlib cannot even start: the device reports it, no bare zlib.error comes out of the peek at its first bytes
    with pytest.raises(pkg.SourmashError) as err:
        ar.ZipCollection(crafted["reserved_block"]).text()
    assert err.value.code == 3 and "reserved block type" in err.value.message and "(entry 0 'r.sig')" in err.value.message
    # a two-member .gz of equal halves is kLeftover exactly
    eq, half = R.equal_halves()
    assert eq == crafted["equal_halves"] and [R.status(eq, e)[1] for e in R.scan(eq)] == [IR.LEFTOVER]
    _, _, status, err = device(pkg, ar, eq)
    assert status.tolist() == [IR.LEFTOVER] and host(ar.ZipCollection(eq).text()[0]) == half + half


def golden_documents():
    paths = sorted(glob.glob(os.path.join(GOLDEN, "sbt_v5", "*.sig"))) + [os.path.join(GOLDEN, "genome-s10+s11.sig")]
    docs = [(os.path.basename(p), open(p, "rb").read()) for p in paths]
    for s in range(6):                                           # scaled sketches as well, for search_many
        sk = SR.sketch_json(sorted(set(range(s, 6000, 3 + s % 4))), ksize=51, max_hash=SR.U64_MAX // 2)
        docs.append(("scaled%d.sig" % s, SR.document([SR.signature_json([sk], name=b'"scaled %d"' % s)])))
    return docs


def golden_zip(docs, manifest):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as z:
        rows = []
        for k, (name, doc) in enumerate(docs):
            if k == 1:
                loc, content, method = "signatures/" + name, doc, zipfile.ZIP_DEFLATED
            elif k == 2:
                loc, content, method = "signatures/" + name, doc, zipfile.ZIP_STORED
            else:
                loc, content, method = "signatures/" + name + ".gz", gzip.compress(doc, mtime=0), zipfile.ZIP_STORED
            z.writestr(zipfile.ZipInfo(loc), content, compress_type=method)
            for sig in json.loads(doc):
                for sk in sig["signatures"]:
                    rows.append({"internal_location": loc, "md5": sk["md5sum"], "md5short": sk["md5sum"][:8], "ksize": sk["ksize"],
                                 "moltype": {"dna": "DNA"}.get(sk.get("molecule", "DNA").lower(), sk.get("molecule", "DNA")),
                                 "num": sk["num"], "scaled": 0, "n_hashes": len(sk["mins"]), "with_abundance": int("abundances" in sk),
                                 "name": sig.get("name") or "", "filename": sig.get("filename") or ""})
        if manifest:
            out = io.StringIO()
            out.write("# SOURMASH-MANIFEST-VERSION: 1.0\n")
            w = csv.DictWriter(out, fieldnames=list(rows[0]))
            w.writeheader()
            w.writerows(rows)
            z.writestr(zipfile.ZipInfo("SOURMASH-MANIFEST.csv"), out.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    return buf.getvalue(), rows


def indexes_equal(a, b):
    (oa, ha, aa), (ob, hb, ab) = a.read(), b.read()
    assert np.array_equal(oa, ob) and np.array_equal(ha, hb)
    assert a.has_abundances == b.has_abundances and (aa is None) == (ab is None)
    if aa is not None:
        assert np.array_equal(aa, ab)
    assert a.max_hash_range == b.max_hash_range and len(a) == len(b)


@pytest.mark.parametrize("manifest", [True, False])
def test_from_zip_equals_the_host_loader(pkg, ar, manifest, tmp_path):
    from sourmash_rust_amd import signature as sg
    RI = pkg.index.ResidentIndex
    docs = golden_documents()
    data, rows = golden_zip(docs, manifest)
    zc = ar.ZipCollection(data)
    assert (zc.manifest is not None) == manifest and [e.kind for e in zc.entries[:4]] == ["gzip", "deflate", "stored", "gzip"]
    if manifest:
        assert len(zc.manifest) == len(rows) == 17 and zc.manifest[0]["internal_location"] == rows[0]["internal_location"]
        assert zc.select() == list(range(len(docs))) and zc.select(ksize=51) == list(range(8, 14)) and zc.select(moltype="protein") == [7]

    def host_route(ksize=0, moltype=None):
        sigs = [s for _, d in docs for s in sg.load_signatures_buffer(d, ksize, moltype)]
        return sigs, [s.first_mh() for s in sigs]
    sigs, mhs = host_route()
    path = tmp_path / "collection.zip"
    path.write_bytes(data)
    for source in (data, str(path), zc):
        dev = RI.from_zip(source)
        indexes_equal(dev, RI(mhs))
        assert [e.name or "" for e in dev.signatures] == [s.name for s in sigs]
    indexes_equal(RI.from_signatures(str(path)), RI(mhs))        # a path whose bytes begin PK\3\4 goes there
    indexes_equal(RI.from_signatures(data, ksize=31), RI(host_route(31)[1]))
    for ksize, moltype in ((31, None), (21, "protein"), (30, "DNA"), (51, "dna"), (0, "protein"), (77, None)):
        want = host_route(ksize, moltype)
        dev = RI.from_zip(zc, ksize=ksize, moltype=moltype)
        assert len(dev) == len(want[1]), (ksize, moltype)
        indexes_equal(dev, RI(want[1]))
        assert [e.name or "" for e in dev.signatures] == [s.name for s in want[0]]
    pick = [rows[3]["md5"], rows[9]["md5"]]
    assert pick[0] != pick[1]
    dev = RI.from_zip(zc, md5=pick)
    indexes_equal(dev, RI([m for m, r in zip(mhs, rows) if r["md5"] in pick]))
    assert len(dev) == sum(r["md5"] in pick for r in rows) >= 2 and len(RI.from_zip(zc, md5=pick[0])) >= 1
    # half of the members through the host: nothing changes
    sizes = sorted(len(d) for _, d in docs)
    limit = sizes[len(sizes) // 2]
    assert 0 < sum(len(d) > limit for _, d in docs) < len(docs)
    indexes_equal(RI.from_zip(zc, device_member_limit=limit), RI(mhs))
    indexes_equal(RI.from_zip(zc, device_member_limit=0), RI(mhs))
    # find and search_many answer alike
    d31, h31 = RI.from_zip(zc, ksize=31), RI(host_route(31)[1])
    for q in host_route(31)[1][:3]:
        assert d31.find(q, 0.0) == h31.find(q, 0.0) and len(d31.find(q, 0.0)) >= 1
        assert d31.find(q, 0.05, containment=True) == h31.find(q, 0.05, containment=True)
    d51, h51 = RI.from_zip(zc, ksize=51), RI(host_route(51)[1])
    a, b = d51.search_many(host_route(51)[1], 0.05), h51.search_many(host_route(51)[1], 0.05)
    assert len(a) > 6 and np.array_equal(a.offsets, b.offsets) and np.array_equal(a.node, b.node) and np.array_equal(a.common, b.common)


# ---------------------------------------------------------------------------------------------------------- stream order
@pytest.mark.parametrize("which", ["caller", "null"])
def test_inflate_dev_is_ordered_on_its_stream(pkg, ar, which):
    """the compressed file is still being produced on the stream: until then the buffer holds an archive of the same layout
    (stored blocks of texts of the same lengths), which inflates without an error to the wrong text"""
    from test_gpu_stream_order import aparts
    stream = aparts(pkg)[0] if which == "caller" else torch.cuda.default_stream()
    handle = SO.handle(stream)
    assert (handle is None) == (which == "null")
    texts = [[pattern(30000 + 1000 * i, 50 * w + i) for i in range(12)] for w in (0, 1)]
    datas = [R.build([R.member("m%d.sig" % i, t, 8, level=0) if i % 2 else R.member("m%d.sig.gz" % i, R.gz(t, 0)) for i, t in enumerate(ts)])
             for ts in texts]
    assert len(datas[0]) == len(datas[1]) and datas[0] != datas[1]
    scans = [[(e.kind, e.payload_off, e.payload_len, e.text_size) for e in R.scan(d)] for d in datas]
    assert scans[0] == scans[1]
    zc = ar.ZipCollection(datas[0])
    true, decoy = (torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas)
    dst = torch.empty_like(true)
    for t in (true, decoy, dst):
        t.record_stream(stream)
    dst.copy_(true)
    torch.cuda.synchronize()
    _, warm, status, err = device(pkg, ar, zc, verify=False, stream=handle, comp=dst)          # (warm-up: the pool has its blocks)
    assert err is None and host(warm) == b"".join(texts[0])
    n = len(zc)
    sizes = [e.text_size for e in zc.entries]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)[:n]
    ids = np.arange(n, dtype=np.uint32)
    out = torch.zeros(sum(sizes), dtype=torch.uint8, device="cuda")
    status = np.zeros(n, dtype=np.uint8)
    torch.cuda.synchronize()
    ev = SO.late(stream, dst, true, decoy)
    SO.pending(ev)
    code = pkg.lib().smh_archive_inflate_dev(zc._p, C.c_void_p(dst.data_ptr()), len(datas[0]), ids.ctypes.data_as(u32p), offs.ctypes.data_as(u64p), n,
                                             C.c_void_p(out.data_ptr()), out.numel(), 0, status.ctypes.data_as(u8p), C.c_void_p(handle or 0))
    assert code == 0 and not status.any()
    assert host(out) == b"".join(texts[0])
    torch.cuda.synchronize()
