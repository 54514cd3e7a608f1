"""Blocked gzip inflated on the device (fastx.inflate, C ABI smh_gzip_*): valid members byte for byte against
zlib / gzip, statuses against tests/inflate_restatement.py -- whose malformed cases and fuzz mutants the host build of the
same decoder has passed under the sanitizers (tests/test_inflate_host.py) -- every block kind, copy shape and size, member
counts under grid caps and the pool fill, a text past 4 GiB, the way through the parser to a sketch, and stream order."""
import ctypes as C
import gzip
import random
import zlib

import numpy as np
import pytest
import torch

import inflate_restatement as R
import stream_order as SO

pytestmark = pytest.mark.gpu

REASON_WORDS = {R.BLOCK_TYPE: "reserved block type", R.STORED_LEN: "NLEN", R.HEADER_COUNTS: "286", R.REPEAT: "repeat",
                R.OVER: "over-subscribed", R.INCOMPLETE: "incomplete", R.NO_EOB: "end-of-block", R.BAD_SYMBOL: "invalid", R.DISTANCE: "distance",
                R.INPUT: "input exhausted", R.OUT_OVER: "pass ISIZE", R.OUT_UNDER: "below ISIZE", R.LEFTOVER: "left over", R.CRC: "CRC"}


@pytest.fixture(scope="module")
def fx(pkg):
    return pkg.fastx


def host(t):
    return bytes(t.cpu().numpy())


def run(pkg, data, verify=True, **kw):
    """(text tensor or None, statuses, error message or None) of one call"""
    status = np.full(len(R.scan(data)), 0xEE, dtype=np.uint8)
    try:
        return pkg.fastx.inflate(data, verify=verify, status=status, **kw), status, None
    except pkg.SourmashError as e:
        assert e.code == 3
        return None, status, e.message


def expect(data, verify=True):
    """(the text of the good members in place, zeros elsewhere; statuses; members)"""
    ms = R.scan(data)
    outs = [R.inflate_member(data, m, verify) for m in ms]
    return ms, [o for o, _ in outs], np.array([r for _, r in outs], dtype=np.uint8)


def check_valid(pkg, data, **kw):
    got, status, err = run(pkg, data, **kw)
    assert err is None and not status.any(), (err, status.nonzero())
    want = gzip.decompress(data) if data else b""
    assert got.dtype == torch.uint8 and got.is_cuda and got.numel() == len(want)
    assert host(got) == want
    return want


# -------------------------------------------------------------------------------------------- block kinds, copies, sizes
def test_every_block_kind_copy_and_size_in_one_call(pkg):
    cases = R.valid_cases()
    names = [n for n, _, _ in cases]
    for need in ("stored", "fixed", "dynamic", "memlevel1", "sync_flush", "full_flush", "huffman_only", "fibonacci", "run_a", "run_ab",
                 "far_repeat", "max_distance", "size_0", "size_1", "size_63", "size_64", "size_65", "size_65280", "size_65535",
                 "size_65536", "noise", "single_code"):
        assert need in names
    noise = next(c for c in cases if c[0] == "noise")
    assert len(noise[1]) > len(noise[2])                       # a payload longer than its output
    data = b"".join(R.member(p, t) for _, p, t in cases) + R.EOF_MEMBER
    want = check_valid(pkg, data)
    assert want == b"".join(t for _, _, t in cases)


def test_end_marker_in_the_middle_and_empty_input(pkg):
    a, b = R.fastq_text(3), R.fastq_text(4, seed=2)
    check_valid(pkg, R.member(R.deflate(a), a) + R.EOF_MEMBER + R.member(R.deflate(b), b) + R.EOF_MEMBER)
    check_valid(pkg, R.EOF_MEMBER)
    got, status, err = run(pkg, b"")
    assert err is None and got.numel() == 0 and status.size == 0


def test_every_output_and_payload_phase(pkg, fx):
    rng = random.Random(3)
    members = []
    for i in range(80):                                        # odd sizes in sequence: members start at every output phase mod 16
        t = bytes(rng.choice(b"ACGT\n") for _ in range(2 * (i % 5) + 1 + 16 * (i % 3)))
        members.append(R.member(R.deflate(t, 6 if i % 3 else 0), t))
    fq = R.fastq_text(6)
    for k in range(8):                                         # FNAME and subfields of 0 .. 7 bytes: payloads at every phase mod 4
        members.append(R.member(R.deflate(fq), fq, name=b"n" * k, extra_before=R.subfield(b"AA", k), extra_after=R.subfield(b"ZZ", 7 - k)))
        members.append(R.member(R.deflate(fq, 6, 8, zlib.Z_FIXED), fq, comment=b"c" * k, hcrc=bool(k & 1)))
    data = b"".join(members)                                   # no end marker: the last payload's trailer ends the bytes
    ms = R.scan(data)
    assert {m.out_off % 16 for m in ms} == set(range(16)) and {m.payload_off % 4 for m in ms} == set(range(4))
    check_valid(pkg, data)
    # the same bytes already in HBM, in a tensor that ends on the last member's last byte
    comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    got = fx.inflate(comp, members=fx.gzip_scan(data))
    assert host(got) == gzip.decompress(data)
    lead = torch.frombuffer(bytearray(b"\xff" * 3 + data), dtype=torch.uint8).cuda()[3:]      # and at an odd address
    assert host(fx.inflate(lead, members=fx.gzip_scan(data))) == gzip.decompress(data)
    with pytest.raises(ValueError):
        fx.inflate(comp)


# ------------------------------------------------------------------------------------------------- member counts and trips
@pytest.fixture(scope="module")
def many():
    rng = random.Random(9)
    out = []
    for i in range(300):
        t = R.fastq_text(2 + i % 3, 40 + i % 17, seed=100 + i) if i % 5 else bytes(rng.choice(b"AC") for _ in range(i))
        out.append(R.member(R.deflate(t, 6, 8, (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY)[i % 3]), t))
    return out


@pytest.mark.parametrize("fill", [-1, 0xA5])
@pytest.mark.parametrize("cap", [0, 1, 3])
def test_member_counts_under_grid_caps_and_pool_fill(pkg, many, cap, fill):
    L = pkg.lib()
    L.smh_set_grid_cap(cap)
    L.smh_set_pool_fill(fill)
    try:
        for n in (1, 2, 64, 65, 300):
            check_valid(pkg, b"".join(many[:n]))
    finally:
        L.smh_set_grid_cap(0)
        L.smh_set_pool_fill(-1)


def test_past_4_gib(pkg, fx):
    block = b"A" * 65536
    one = R.member(R.deflate(block), block)
    assert len(one) < 200
    tail = bytes(range(256)) * 3
    last = R.member(R.deflate(tail), tail)
    n = 65540
    data = one * (n - 1) + last
    g = fx.gzip_scan(data)
    assert len(g) == n and g.inflated_len == (n - 1) * 65536 + len(tail) > 1 << 32
    status = np.full(n, 0xEE, dtype=np.uint8)
    out = fx.inflate(data, status=status)
    assert not status.any() and out.numel() == g.inflated_len
    edge = 1 << 32
    assert bool((out[edge - 70000:edge + 70000] == 65).all())
    assert bool((out[:65536] == 65).all()) and bool((out[(n - 2) * 65536:(n - 1) * 65536] == 65).all())
    assert host(out[(n - 1) * 65536:]) == tail
    assert int((out != 65).sum()) == sum(1 for b in tail if b != 65)
    del out


# ------------------------------------------------------------------------------------------------------------ malformed
def malformed_batch():
    """members, some good and most bad, and their names"""
    good_text = R.fastq_text(4, seed=8)
    good = R.member(R.deflate(good_text), good_text)
    members, names = [good], ["good_first"]
    for name, payload, isize, _ in R.malformed_cases():
        members.append(R.member(payload, isize))
        names.append(name)
        members.append(good)
        names.append("good_after_" + name)
    for i, (p, isize, crc) in enumerate(R.fuzz_mutants()[:300]):
        members.append(R.member(p, isize, crc))
        names.append("fuzz_%d" % i)
    members.append(good)
    names.append("good_last")
    return members, names


def test_malformed_members_one_status_each(pkg):
    members, names = malformed_batch()
    data = b"".join(members)
    for verify in (True, False):
        ms, outs, want = expect(data, verify)
        assert len(set(want.tolist())) >= 12                   # (the batch reaches most reasons)
        got, status, err = run(pkg, data, verify=verify)
        bad = [(names[i], int(status[i]), int(want[i])) for i in range(len(ms)) if status[i] != want[i]]
        assert not bad, bad[:10]
        low = int(np.nonzero(want)[0][0])
        assert got is None and "(member %d at byte %d)" % (low, ms[low].header_off) in err and REASON_WORDS[int(want[low])] in err, err
    # the malformed cases alone carry no CRC: without verification the reasons are the restatement's own
    for (name, payload, isize, reason), w in zip(R.malformed_cases(), want[1::2]):
        assert w == reason, name


def test_good_members_next_to_bad_ones_are_right(pkg, fx):
    members, names = malformed_batch()
    data = b"".join(members)
    ms, outs, want = expect(data)
    comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    g = fx.gzip_scan(data)
    out = torch.full((g.inflated_len + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    status = np.zeros(len(ms), dtype=np.uint8)
    code = pkg.lib().smh_gzip_inflate_dev(g._p, C.c_void_p(comp.data_ptr()), len(data), C.c_void_p(out.data_ptr()), g.inflated_len, 1,
                                          status.ctypes.data_as(C.POINTER(C.c_uint8)), None)
    assert code == 3 and np.array_equal(status, want)
    text = host(out)
    assert text[g.inflated_len:] == b"\x5a" * 64               # nothing behind the text is written
    for m, o, w in zip(ms, outs, want):
        if w == R.OK:
            assert text[m.out_off:m.out_off + m.isize] == o


def test_one_flipped_crc_byte(pkg):
    texts = [R.fastq_text(3, seed=40 + i) for i in range(10)]
    j = 6
    members = [R.member(R.deflate(t), t, crc=zlib.crc32(t) ^ (0x4000 if i == j else 0)) for i, t in enumerate(texts)]
    data = b"".join(members)
    got, status, err = run(pkg, data)
    assert got is None and status.tolist() == [0] * j + [R.CRC] + [0] * (9 - j)
    assert "(member %d at byte %d)" % (j, sum(len(m) for m in members[:j])) in err and "CRC" in err
    got, status, err = run(pkg, data, verify=False)
    assert err is None and not status.any() and host(got) == b"".join(texts)


def test_arguments_are_checked(pkg, fx):
    data = R.bgzf(R.fastq_text(3))
    g = fx.gzip_scan(data)
    comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = torch.zeros(g.inflated_len, dtype=torch.uint8, device="cuda")
    L = pkg.lib()
    assert L.smh_gzip_inflate_dev(g._p, C.c_void_p(comp.data_ptr()), len(data), C.c_void_p(out.data_ptr()), g.inflated_len - 1, 1, None, None) == 3
    assert L.smh_gzip_inflate_dev(g._p, C.c_void_p(comp.data_ptr()), len(data) - 1, C.c_void_p(out.data_ptr()), g.inflated_len, 1, None, None) == 3
    assert not out.any()


# ---------------------------------------------------------------------------------------------------- through the stack
def wrapped_fasta(rng, n):
    out = []
    for i in range(n):
        seq = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(3000, 9000)))
        out.append(b">contig%d some words\r\n" % i + b"".join(seq[k:k + 70] + b"\r\n" for k in range(0, len(seq), 70)))
    return b"".join(out)


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_parse_bgzf_equals_parse(pkg, fx, fmt):
    rng = random.Random(17)
    text = wrapped_fasta(rng, 30) if fmt == "fasta" else R.fastq_text(600, 150, seed=5)
    assert len(text) > 2 * 65280                               # records and \r\n pairs straddle members
    data = R.bgzf(text, 65280)
    plain = fx.Records.parse(text)
    recs = fx.Records.parse_bgzf(data, keep_text=True)
    assert recs.format == plain.format == fmt and len(recs) == len(plain) and recs.total == plain.total
    assert np.array_equal(recs.offsets, plain.offsets)
    assert torch.equal(recs.seq_tensor(), plain.seq_tensor())
    for a, b in zip(recs.name_spans(), plain.name_spans()):
        assert np.array_equal(a, b)
    assert recs.names() == plain.names(text) and len(recs.names()) == len(recs)
    assert host(recs.text) == text
    bare = fx.Records.parse_bgzf(data)
    assert bare.text is None and bare.names(text) == plain.names(text)
    with pytest.raises(ValueError):
        bare.names()
    a, b = pkg.KmerMinHash(0, 21, False, 42, (1 << 64) // 20, True), pkg.KmerMinHash(0, 21, False, 42, (1 << 64) // 20, True)
    a.add_records(recs, True)
    b.add_records(plain, True)
    assert a.mins == b.mins and a.abunds == b.abunds and len(a.mins) > 100


def test_read_device_text_routes(pkg, fx, tmp_path):
    text = R.fastq_text(300, 150, seed=6)
    paths = {"bgzf": (tmp_path / "r.fastq.bgz", R.bgzf(text, 30000)), "gz": (tmp_path / "r.fastq.gz", gzip.compress(text)),
             "plain": (tmp_path / "r.fastq", text), "empty": (tmp_path / "e.fastq", b"")}
    for p, raw in paths.values():
        p.write_bytes(raw)
    assert fx.is_bgzf(paths["bgzf"][1]) and not fx.is_bgzf(paths["gz"][1])
    got = {k: fx.read_device_text(str(p)) for k, (p, _) in paths.items()}
    assert all(t.is_cuda and t.dtype == torch.uint8 for t in got.values())
    assert host(got["bgzf"]) == text and torch.equal(got["bgzf"], got["gz"]) and torch.equal(got["gz"], got["plain"])
    assert got["empty"].numel() == 0
    assert fx.read_text(str(paths["bgzf"][0])) == text         # the host route reads the same file
    mixed = tmp_path / "mixed.gz"                              # a blocked member, then a plain one: "not blocked gzip", so the host
    mixed.write_bytes(R.bgzf(text[:5000], eof=False) + gzip.compress(text[5000:]))
    assert host(fx.read_device_text(str(mixed))) == text
    broken = tmp_path / "broken.bgz"                           # any other refusal is the caller's to see
    broken.write_bytes(R.bgzf(text)[:-5])
    with pytest.raises(pkg.SourmashError):
        fx.read_device_text(str(broken))


# ---------------------------------------------------------------------------------------------------------- stream order
@pytest.mark.parametrize("which", ["caller", "null"])
def test_inflate_dev_is_ordered_on_its_stream(pkg, fx, which):
    """the compressed bytes are still being produced on the stream: until then the buffer holds other members of the same
    layout (stored blocks of a text of the same length), which inflate without an error to the wrong text"""
    from test_gpu_stream_order import aparts
    stream = aparts(pkg)[0] if which == "caller" else torch.cuda.default_stream()
    handle = SO.handle(stream)
    assert (handle is None) == (which == "null")
    texts = [R.fastq_text(200, 100, seed=s) for s in (71, 72)]
    assert len(texts[0]) == len(texts[1]) and texts[0] != texts[1]
    datas = [R.bgzf(t, 20000, level=0) for t in texts]
    assert len(datas[0]) == len(datas[1])
    assert [m[1:4] for m in R.scan(datas[0])] == [m[1:4] for m in R.scan(datas[1])]
    g = fx.gzip_scan(datas[0])
    true, decoy = (torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas)
    dst = torch.empty_like(true)
    for t in (true, decoy, dst):
        t.record_stream(stream)
    dst.copy_(true)
    torch.cuda.synchronize()
    assert host(fx.inflate(dst, verify=False, members=g, stream=handle)) == texts[0]         # (warm-up: the pool has its blocks)
    ev = SO.late(stream, dst, true, decoy)
    SO.pending(ev)
    got = fx.inflate(dst, verify=False, members=g, stream=handle)
    assert host(got) == texts[0]
    torch.cuda.synchronize()
