"""The rules of zip collections (tests/archive_restatement.py), pinned: the restated scan against Python's
zipfile on valid archives of every shape, its refusal on each crafted one, and the chunked CRC fold against zlib.crc32.
No GPU and nothing from the package."""
import io
import struct
import zipfile
import zlib

import pytest

import archive_restatement as R

CRAFTED = dict(R.crafted())


def by_zipfile(data):
    """[(name, method, flags, crc, compressed size, size, header offset, content)] as zipfile sees the archive"""
    out = []
    with zipfile.ZipFile(io.BytesIO(data)) as z:
        for info in z.infolist():
            content = z.read(info) if info.compress_type in (0, 8) and not info.flag_bits & 1 else None
            out.append((info.filename.encode(), info.compress_type, info.flag_bits, info.CRC, info.compress_size, info.file_size,
                        info.header_offset, content))
    return out


def content_of(data, e):
    raw = data[e.data_off:e.data_off + e.comp_size]
    return zlib.decompress(raw, -15) if e.method == 8 else raw


def check_against_zipfile(data):
    got, want = R.scan(data), by_zipfile(data)
    assert len(got) == len(want)
    for e, (name, method, flags, crc, cs, size, off, content) in zip(got, want):
        assert (e.name, e.method, e.flags, e.crc32, e.comp_size, e.size, e.header_off) == (name, method, flags, crc, cs, size, off)
        if content is not None:
            assert content_of(data, e) == content
    return got


def written_by_zipfile(members, **kw):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", **kw) as z:
        for name, content, method in members:
            z.writestr(zipfile.ZipInfo(name), content, compress_type=method)
    return buf.getvalue()


@pytest.mark.parametrize("name", ["three", "empty", "directories", "descriptor", "local_extra_longer", "comment_plain", "zip64_extra",
                                  "zip64_extra_behind_another", "zip64_end", "empty_zip64", "entry_comment", "gzip_fields", "doubly_compressed"])
def test_valid_archives_as_zipfile_reads_them(name):
    got = check_against_zipfile(CRAFTED[name])
    assert all(e.device_ok for e in got), [e.reason for e in got]


def test_kinds_come_from_content():
    a, b, c = R.gz(R.sig_text(1)), R.sig_text(2), R.sig_text(3)
    data = R.build([R.member("looks-plain.sig", a), R.member("looks-gz.sig.gz", c), R.member("deflated.bin", b, 8), R.member("d/", b""),
                    R.member("odd/", b"xy"), R.member("x.bz2", c, 12)])
    got = check_against_zipfile(data)
    assert [e.kind for e in got] == [R.GZIP, R.STORED, R.DEFLATE, R.DIRECTORY, R.STORED, R.OTHER]
    g = got[0]
    assert (g.text_size, g.text_crc) == (len(R.sig_text(1)), zlib.crc32(R.sig_text(1)))
    assert zlib.decompress(data[g.payload_off:g.payload_off + g.payload_len], -15) == R.sig_text(1)
    assert data[g.payload_off + g.payload_len:][:8] == struct.pack("<II", g.text_crc, g.text_size)
    for e in got[1:5]:
        assert (e.payload_off, e.payload_len, e.text_size, e.text_crc) == (e.data_off, e.comp_size, e.size, e.crc32)


def test_the_local_headers_own_lengths_give_the_data_offset():
    data = CRAFTED["local_name_longer"]                          # (zipfile refuses names that differ; the data is where it is)
    b, c = R.scan(data)
    assert (b.name, c.name) == (b"b.sig", b"c.sig")
    assert content_of(data, b) == R.sig_text(2) and content_of(data, c) == R.sig_text(3)
    assert b.data_off - b.header_off == 30 + len(b"another-name.sig") and c.data_off - c.header_off == 30


def test_gzip_header_fields():
    data = CRAFTED["gzip_fields"]
    for k, e in enumerate(R.scan(data)):
        assert e.kind == R.GZIP and e.device_ok
        assert zlib.decompress(data[e.payload_off:e.payload_off + e.payload_len], -15) == R.sig_text(10 + k)


def test_archives_written_by_zipfile():
    texts = [R.sig_text(20 + i, 30 + i) for i in range(5)]
    members = [("signatures/%d.sig.gz" % i, R.gz(t), zipfile.ZIP_STORED) for i, t in enumerate(texts)]
    members += [("plain.sig", texts[0], zipfile.ZIP_STORED), ("deflated.sig", texts[1], zipfile.ZIP_DEFLATED), ("dir/", b"", zipfile.ZIP_STORED)]
    data = written_by_zipfile(members)
    got = check_against_zipfile(data)
    assert [e.kind for e in got] == [R.GZIP] * 5 + [R.STORED, R.DEFLATE, R.DIRECTORY]
    # force_zip64: the local headers carry a zip64 extra field the central directory does not have
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as z:
        for i, t in enumerate(texts):
            with z.open(zipfile.ZipInfo("f%d.sig" % i), "w", force_zip64=True) as fh:
                fh.write(t)
    data = buf.getvalue()
    got = check_against_zipfile(data)
    assert all(e.data_off - e.header_off > 30 + len(e.name) for e in got)
    assert [content_of(data, e) for e in got] == texts
    # a streamed member: zipfile writes a data descriptor when the file cannot seek
    class NoSeek(io.RawIOBase):
        def __init__(self): self.b = bytearray()
        def writable(self): return True
        def write(self, x):
            self.b += x
            return len(x)
    sink = NoSeek()
    with zipfile.ZipFile(sink, "w") as z:
        z.writestr("streamed.sig", texts[2], compress_type=zipfile.ZIP_DEFLATED)
    data = bytes(sink.b)
    got = check_against_zipfile(data)
    assert got[0].flags & 8 and content_of(data, got[0]) == texts[2]


def test_zip64_from_65536_empty_entries():
    data = written_by_zipfile([("e%05d" % i, b"", zipfile.ZIP_STORED) for i in range(65536)])
    assert b"PK\6\6" in data and b"PK\6\7" in data
    got = R.scan(data)
    assert len(got) == 65536 and got[65535].name == b"e65535" and all(e.kind == R.STORED and e.size == 0 for e in got[::997])
    with zipfile.ZipFile(io.BytesIO(data)) as z:
        assert [i.header_offset for i in z.infolist()] == [e.header_off for e in got]


def test_a_comment_with_an_end_record_does_not_fool_the_scan():
    want = R.scan(CRAFTED["three"])
    for name in ("comment_plain", "comment_with_signature", "comment_with_end_record"):
        assert R.scan(CRAFTED[name]) == want, name
    # (not compared with zipfile here: the versions that take the LAST signature in the window are fooled by this comment)


def test_every_truncation_is_refused():
    data = R.three()
    for k in range(len(data)):
        with pytest.raises(R.Refused, match="^archive: "):
            R.scan(data[:k])


@pytest.mark.parametrize("name", sorted(R.REFUSALS))
def test_refusals(name):
    with pytest.raises(R.Refused) as err:
        R.scan(CRAFTED[name])
    msg = str(err.value)
    assert msg.startswith("archive: " + R.REFUSALS[name] + " ("), msg
    assert ("at byte " in msg) and (("(entry " in msg) == (name in ("multi_disk_entry", "cd_truncated_count", "cd_truncated_size", "cd_signature",
                                                                     "local_signature", "zip64_extra_missing", "zip64_extra_short", "data_outside",
                                                                     "local_outside"))), msg


def test_refusals_name_the_entry_and_byte():
    data = CRAFTED["local_signature"]
    with pytest.raises(R.Refused, match=r"\(entry 0 at byte 0\)"):
        R.scan(data)
    three = R.three()
    second = three.index(b"PK\3\4", 4)
    with pytest.raises(R.Refused, match=r"local header without its signature \(entry 1 at byte %d\)" % second):
        R.scan(three[:second] + b"PK\3\5" + three[second + 4:])
    with pytest.raises(R.Refused, match=r"truncated central directory \(entry 3 at byte %d\)" % three.index(b"PK\5\6")):
        R.scan(CRAFTED["cd_truncated_count"])


@pytest.mark.parametrize("name,reasons", [("encrypted", ["encrypted entry", ""]), ("method_12", ["compression method 12", ""]),
                                          ("stored_sizes_differ", ["stored entry whose sizes differ"]), ("size_2_32", ["size of 2^32 or more"]),
                                          ("gzip_short", ["gzip entry shorter than its header and trailer"]),
                                          ("gzip_header_cut", ["gzip entry shorter than its header and trailer"])])
def test_entries_the_device_does_not_take_are_still_listed(name, reasons):
    got = R.scan(CRAFTED[name])
    assert [e.reason for e in got] == reasons and [e.device_ok for e in got] == [not r for r in reasons]
    assert all(R.status(CRAFTED[name], e)[1] == (R.NOT_RUN if e.reason else R.IR.OK) for e in got)


def test_statuses_of_the_bad_members():
    for name, want in (("wrong_crc", [R.IR.CRC, R.IR.CRC]), ("wrong_trailer", [R.IR.CRC]), ("gzip_two_members", [R.IR.LEFTOVER])):
        data = CRAFTED[name]
        assert [R.status(data, e)[1] for e in R.scan(data)] == want, name
    data = CRAFTED["flipped_payload"]
    assert R.status(data, R.scan(data)[0])[1] != R.IR.OK
    data = CRAFTED["wrong_crc"]
    assert [R.status(data, e, verify=False)[1] for e in R.scan(data)] == [R.IR.OK, R.IR.OK]


# ------------------------------------------------------------------------------------------------ the fold
def test_table_arithmetic_is_zlibs():
    text = bytes(range(256)) * 3 + b"tail"
    assert R.crc_run(0xFFFFFFFF, text) ^ 0xFFFFFFFF == zlib.crc32(text)
    assert R.zlib_run(0, text) == R.crc_run(0, text) and R.zlib_run(0x1234, text) == R.crc_run(0x1234, text)
    for n in (0, 1, 7, 300):
        assert R.crc_shift(0xDEADBEEF, n) == R.crc_run(0xDEADBEEF, bytes(n))


@pytest.mark.parametrize("size", [0, 1, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 2 * R.CHUNK + 1, 65 * R.CHUNK + 1, 65536, 65537, (1 << 20) + 1])
def test_fold_of_chunk_registers_is_the_crc(size):
    text = bytes((i * 13 + (i >> 7)) & 0xFF for i in range(size))
    terms = R.chunk_terms(text, R.zlib_run)
    assert len(terms) == R.chunks_of(size) == (size + R.CHUNK - 1) // R.CHUNK
    assert R.fold(terms, size) == zlib.crc32(text)
    if size <= R.CHUNK + 1:
        assert R.chunk_terms(text) == terms                      # the table-driven run, where it is quick


def test_member_of_chunk_steps_over_members_without_chunks():
    sizes = [0, 1, 0, 0, R.CHUNK, R.CHUNK + 1, 0, 3 * R.CHUNK, 0]
    prefix = [0]
    for s in sizes:
        prefix.append(prefix[-1] + R.chunks_of(s))
    owner = [m for m, s in enumerate(sizes) for _ in range(R.chunks_of(s))]
    assert [R.member_of_chunk(prefix, w) for w in range(prefix[-1])] == owner
