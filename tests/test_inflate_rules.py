"""The blocked-gzip rules without a GPU: tests/inflate_restatement.py pinned to zlib (crafted members and a seeded fuzz), the
scan rules in the restatement and in the library, and the inflate calls' error without a device."""
import ctypes as C
import gzip
import struct
import zlib

import pytest

import inflate_restatement as R


def zlib_verdict(payload):
    """("ok", bytes) when zlib accepts the payload as one complete raw stream of at most 65 536 bytes with nothing behind
    it, ("bad", None) when it raises, ("open", None) otherwise (it wants more input, has input left, or too much output)"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload)
    except zlib.error:
        return "bad", None
    if d.eof and not d.unused_data and len(out) <= R.MAX_MEMBER:
        return "ok", out
    return "open", None


def test_valid_cases_decode_like_zlib():
    for name, payload, text in R.valid_cases():
        verdict, out = zlib_verdict(payload)
        assert verdict == "ok" and out == text, name
        got, reason = R.inflate_payload(payload, len(text), zlib.crc32(text))
        assert reason == R.OK and got == text, (name, reason)


def test_malformed_cases_have_their_reason_and_zlib_rejects_them():
    unseen = (R.OUT_OVER, R.OUT_UNDER, R.LEFTOVER)      # what only the trailer shows: zlib decodes these payloads
    for name, payload, isize, want in R.malformed_cases():
        got, reason = R.inflate_payload(payload, isize)
        assert reason == want, (name, reason)
        verdict, _ = zlib_verdict(payload)
        if want == R.INPUT:
            assert verdict == "open", name
        elif want == R.LEFTOVER:
            assert zlib.decompressobj(-15).decompress(payload) == got and verdict == "open", name
        elif want in unseen:
            assert verdict == "ok", name
        else:
            assert verdict == "bad", name


def test_crc_is_checked_last_and_only_when_asked():
    text = R.fastq_text(5)
    payload = R.deflate(text)
    assert R.inflate_payload(payload, len(text), zlib.crc32(text) ^ 0x100) == (text, R.CRC)
    assert R.inflate_payload(payload, len(text), None) == (text, R.OK)


def test_fuzz_agrees_with_zlib():
    seen = {"ok": 0, "bad": 0, "open": 0}
    reasons = set()
    for payload, isize, crc in R.fuzz_mutants():
        verdict, out = zlib_verdict(payload)
        got, reason = R.inflate_stream(payload)
        seen[verdict] += 1
        reasons.add(reason)
        if verdict == "ok":
            assert reason == R.OK and got == out
        elif verdict == "bad":
            assert reason != R.OK
    assert seen["ok"] > 20 and seen["bad"] > 500            # the fuzz reaches both sides
    assert len(reasons) >= 8


# ------------------------------------------------------------------------------------------------------------- the scan
def _scan_cases():
    text = b">a\nACGT\n"
    p = R.deflate(text)
    ok = []
    for flags in range(16):                                  # FNAME, FCOMMENT, FHCRC, a subfield in front of BC
        ok.append(R.member(p, text, name=b"n.fa" if flags & 1 else None, comment=b"c c" if flags & 2 else None, hcrc=bool(flags & 4),
                           extra_before=R.subfield(b"XY", 3) if flags & 8 else b"", extra_after=R.subfield(b"ZZ", flags & 3)))
    return text, p, ok


def _refusals():
    text, p, ok = _scan_cases()
    m = ok[0]
    plain = gzip.compress(text)
    big = R.member(p, 65537)
    return [("not gzip", b"hello world, this is text", 0, 0),
            ("not gzip", b"\x1f\x8b\x07" + m[3:], 0, 0),
            ("not blocked gzip", plain, 0, 0),
            ("not blocked gzip", m + plain, 1, len(m)),
            ("BSIZE", m[:-1], 0, 0),
            ("BSIZE", m + m[:len(m) - 3], 1, len(m)),
            ("cut short", m[:7], 0, 0),
            ("cut short", m[:11], 0, 0),
            ("cut short", m + b"\x1f", 1, len(m)),
            ("cut short", R.member(p, text, name=b"x" * 10)[:20], 0, 0),
            ("ISIZE", big, 0, 0),
            ("trail", m + b"\0\0\0", 1, len(m)),
            ("trail", m + R.EOF_MEMBER + b"garbage", 2, len(m) + len(R.EOF_MEMBER))]


def test_restatement_scan():
    text, p, ok = _scan_cases()
    assert R.scan(b"") == []
    chain = b"".join(ok) + R.EOF_MEMBER
    ms = R.scan(chain)
    assert len(ms) == 17 and [m.isize for m in ms] == [len(text)] * 16 + [0]
    assert [m.out_off for m in ms] == [len(text) * i for i in range(17)]
    for m in ms[:16]:
        assert chain[m.payload_off:m.payload_off + m.payload_len] == p and m.crc == zlib.crc32(text)
    assert gzip.decompress(chain) == text * 16
    for what, data, index, off in _refusals():
        with pytest.raises(R.ScanError) as ei:
            R.scan(data)
        assert (ei.value.index, ei.value.offset) == (index, off), what
        assert {"not gzip": "not gzip", "not blocked gzip": "not blocked", "BSIZE": "BSIZE", "cut short": "cut short", "ISIZE": "ISIZE",
                "trail": "trail"}[what] in ei.value.what, (what, ei.value.what)


def test_library_scan_agrees_with_the_restatement(pkg):
    from sourmash_rust_amd import fastx
    text, p, ok = _scan_cases()
    chain = b"".join(ok) + R.EOF_MEMBER
    assert len(fastx.gzip_scan(b"")) == 0 and fastx.gzip_scan(b"").inflated_len == 0
    g = fastx.gzip_scan(chain)
    ms = R.scan(chain)
    assert len(g) == len(ms) and g.inflated_len == sum(m.isize for m in ms)
    assert [g.member(i) for i in range(len(g))] == [(m.payload_off, m.payload_len, m.isize, m.crc) for m in ms]
    assert fastx.is_bgzf(chain) and not fastx.is_bgzf(gzip.compress(text)) and not fastx.is_bgzf(text) and not fastx.is_bgzf(b"")
    for what, data, index, off in _refusals():
        with pytest.raises(pkg.SourmashError) as ei:
            fastx.gzip_scan(data)
        assert ei.value.code == 3, what
        assert "member %d at byte %d" % (index, off) in ei.value.message, (what, ei.value.message)
        assert {"not gzip": "not gzip", "not blocked gzip": "not blocked gzip", "BSIZE": "BSIZE", "cut short": "cut short",
                "ISIZE": "ISIZE", "trail": "trail"}[what] in ei.value.message, (what, ei.value.message)
    with pytest.raises(pkg.SourmashError):
        g.member(len(g))


def test_inflate_fails_loudly_without_gpu(pkg):
    if pkg.device_available():
        pytest.skip("a GPU is present")
    from sourmash_rust_amd import fastx
    L = pkg.lib()
    data = R.bgzf(b">a\nACGT\n")
    with pytest.raises(pkg.SourmashError) as ei:
        fastx.inflate(data)
    assert ei.value.code == 2
    g = fastx.gzip_scan(data)
    assert L.smh_gzip_inflate_dev(g._p, None, len(data), None, g.inflated_len, 1, None, None) == 2
    assert L.smh_gzip_inflate(data, len(data), None, g.inflated_len, 1, None) == 2
    with pytest.raises(pkg.SourmashError) as ei:
        fastx.Records.parse_bgzf(data)
    assert ei.value.code == 2
