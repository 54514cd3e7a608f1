"""Zip collections restated (include/sourmash_amd.h, "Zip collections"): the scan of the container and the
chunked CRC-32 fold in plain Python, with struct and integers only -- no zipfile, nothing from the package.  It is normative:
the library's scan (csrc/archive_core.hpp) must give these entries and these refusals, word for word.

    scan(data)                 [Entry], or raises Refused("archive: ...")
    chunk_terms / fold         the CRC-32 of a text from the registers of its chunks
    build(members, ...)        a zip written by hand, every field settable (the crafted cases)
    crafted() / mutants()      the archives the host build and the device are tested on

A member's inflate status is inflate_restatement's (the decoder is the same one)."""
import random
import struct
import zlib
from collections import namedtuple

import inflate_restatement as IR

CHUNK = 16384
STORED, DEFLATE, GZIP, DIRECTORY, OTHER = range(5)
NOT_RUN = 0xFF                                                   # status of an entry the device does not take

Entry = namedtuple("Entry", "name method flags crc32 comp_size size header_off data_off kind device_ok reason payload_off payload_len "
                            "text_size text_crc")


class Refused(Exception):
    pass


def _le16(d, p): return d[p] | d[p + 1] << 8
def _le32(d, p): return _le16(d, p) | _le16(d, p + 2) << 16
def _le64(d, p): return _le32(d, p) | _le32(d, p + 4) << 32
def _sig(d, p, a, b): return d[p] == 0x50 and d[p + 1] == 0x4B and d[p + 2] == a and d[p + 3] == b
def _at(off): return " (at byte %d)" % off
def _ate(i, off): return " (entry %d at byte %d)" % (i, off)


def gzip_header(h, left):
    """the first byte behind the RFC 1952 header of h[:left] (which begins 1f 8b 08), or None when the header or the trailer's
    8 bytes behind it do not fit"""
    if left < 10:
        return None
    flg, at = h[3], 10
    if flg & 4:
        if left - at < 2:
            return None
        xlen = _le16(h, at)
        at += 2
        if left - at < xlen:
            return None
        sub, end = at, at + xlen
        while sub < end:
            if end - sub < 4:
                return None
            slen = _le16(h, sub + 2)
            if end - sub - 4 < slen:
                return None
            sub += 4 + slen
        at = end
    for bit in (8, 16):
        if not flg & bit:
            continue
        while at < left and h[at] != 0:
            at += 1
        if at >= left:
            return None
        at += 1
    if flg & 2:
        at += 2
    if at > left or left - at < 8:
        return None
    return at


def classify(d, name, method, flags, crc32, comp_size, size, header_off, data_off):
    if name and name[-1:] == b"/" and size == 0:
        kind = DIRECTORY
    elif method == 8:
        kind = DEFLATE
    elif method == 0:
        kind = GZIP if comp_size >= 3 and d[data_off:data_off + 3] == b"\x1f\x8b\x08" else STORED
    else:
        kind = OTHER

    def entry(ok, reason, payload_off=data_off, payload_len=0, text_size=0, text_crc=crc32):
        return Entry(name, method, flags, crc32, comp_size, size, header_off, data_off, kind, ok, reason, payload_off, payload_len, text_size,
                     text_crc)
    if flags & 1:
        return entry(False, "encrypted entry")
    if kind == OTHER:
        return entry(False, "compression method %d" % method)
    if comp_size >> 32 or size >> 32:
        return entry(False, "size of 2^32 or more")
    if kind == DIRECTORY:
        return entry(True, "")
    if method == 0 and comp_size != size:
        return entry(False, "stored entry whose sizes differ")
    if kind == GZIP:
        h = d[data_off:data_off + comp_size]
        at = gzip_header(h, comp_size)
        if at is None:
            return entry(False, "gzip entry shorter than its header and trailer")
        return entry(True, "", data_off + at, comp_size - at - 8, _le32(h, comp_size - 4), _le32(h, comp_size - 8))
    return entry(True, "", data_off, comp_size, size, crc32)


def scan(data):
    d, n_bytes = bytes(data), len(data)

    def refuse(why):
        raise Refused("archive: " + why)
    if n_bytes < 22:
        refuse("no end-of-central-directory record" + _at(n_bytes))
    eocd = None
    p = n_bytes - 22
    while True:                                                  # the LOWEST consistent place of the window
        if _sig(d, p, 5, 6) and _le16(d, p + 20) == n_bytes - 22 - p:
            eocd = p
        if p == 0 or n_bytes - 22 - p == 65535:
            break
        p -= 1
    if eocd is None:
        refuse("no end-of-central-directory record" + _at(n_bytes))
    disk, cd_disk, n_here, n = _le16(d, eocd + 4), _le16(d, eocd + 6), _le16(d, eocd + 8), _le16(d, eocd + 10)
    cd_size, cd_off, limit = _le32(d, eocd + 12), _le32(d, eocd + 16), eocd
    if eocd >= 20 and _sig(d, eocd - 20, 6, 7):
        loc = eocd - 20
        if _le32(d, loc + 4) != 0 or _le32(d, loc + 16) > 1:
            refuse("multi-disk archive" + _at(loc))
        z = _le64(d, loc + 8)
        if z > n_bytes or n_bytes - z < 56 or not _sig(d, z, 6, 6):
            refuse("zip64 end record outside the data or without its signature" + _at(z))
        disk, cd_disk, n_here, n = _le32(d, z + 16), _le32(d, z + 20), _le64(d, z + 24), _le64(d, z + 32)
        cd_size, cd_off, limit = _le64(d, z + 40), _le64(d, z + 48), z
    if disk != 0 or cd_disk != 0 or n_here != n:
        refuse("multi-disk archive" + _at(eocd))
    if cd_off > limit or cd_size > limit - cd_off:
        refuse("central directory outside the data" + _at(cd_off))
    cd_end, at, out = cd_off + cd_size, cd_off, []
    i = 0
    while i < n:
        if cd_end - at < 46:
            refuse("truncated central directory" + _ate(i, at))
        if not _sig(d, at, 1, 2):
            refuse("central directory entry without its signature" + _ate(i, at))
        nlen, xlen, clen = _le16(d, at + 28), _le16(d, at + 30), _le16(d, at + 32)
        if cd_end - at - 46 < nlen + xlen + clen:
            refuse("truncated central directory" + _ate(i, at))
        flags, method, crc32 = _le16(d, at + 8), _le16(d, at + 10), _le32(d, at + 16)
        comp_size, size, header_off, disk_start = _le32(d, at + 20), _le32(d, at + 24), _le32(d, at + 42), _le16(d, at + 34)
        name = d[at + 46:at + 46 + nlen]
        if size == 0xFFFFFFFF or comp_size == 0xFFFFFFFF or header_off == 0xFFFFFFFF or disk_start == 0xFFFF:
            x, k, found = at + 46 + nlen, 0, False
            while xlen - k >= 4:
                fid, sz = _le16(d, x + k), _le16(d, x + k + 2)
                if sz > xlen - k - 4:
                    break
                if fid == 1:
                    q, left, found = x + k + 4, sz, True
                    if size == 0xFFFFFFFF:
                        if left < 8:
                            found = False
                            break
                        size, q, left = _le64(d, q), q + 8, left - 8
                    if comp_size == 0xFFFFFFFF:
                        if left < 8:
                            found = False
                            break
                        comp_size, q, left = _le64(d, q), q + 8, left - 8
                    if header_off == 0xFFFFFFFF:
                        if left < 8:
                            found = False
                            break
                        header_off, q, left = _le64(d, q), q + 8, left - 8
                    if disk_start == 0xFFFF:
                        if left < 4:
                            found = False
                            break
                        disk_start = _le32(d, q)
                    break
                k += 4 + sz
            if not found:
                refuse("zip64 extra field missing or cut short" + _ate(i, at))
        if disk_start != 0:
            refuse("multi-disk archive" + _ate(i, at))
        lh = header_off
        if lh > n_bytes or n_bytes - lh < 30:
            refuse("local header outside the data" + _ate(i, lh))
        if not _sig(d, lh, 3, 4):
            refuse("local header without its signature" + _ate(i, lh))
        data_off = lh + 30 + _le16(d, lh + 26) + _le16(d, lh + 28)
        if data_off > n_bytes or comp_size > n_bytes - data_off:
            refuse("entry data outside the data" + _ate(i, data_off))
        out.append(classify(d, name, method, flags, crc32, comp_size, size, header_off, data_off))
        at += 46 + nlen + xlen + clen
        i += 1
    return out


# ------------------------------------------------------------------------------------------------ CRC-32 in chunks
POLY = 0xEDB88320
_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ POLY if _c & 1 else _c >> 1
    _TABLE.append(_c)


def crc_run(state, data):
    for b in data:
        state = _TABLE[(state ^ b) & 0xFF] ^ (state >> 8)
    return state


def crc_mul(a, b):
    p = 0
    for k in range(32):
        if a & (0x80000000 >> k):
            p ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return p


def crc_shift(state, n):
    """state * x^(8 n): the register after n more zero bytes"""
    pw, base = 0x80000000, 0x00800000
    while n:
        if n & 1:
            pw = crc_mul(pw, base)
        base = crc_mul(base, base)
        n >>= 1
    return crc_mul(state, pw)


def chunks_of(size): return (size + CHUNK - 1) // CHUNK
def chunk_begin(size, c): return min(c * CHUNK, size)


def member_of_chunk(prefix, w):
    """the last m with prefix[m] <= w (prefix: one more entry than members)"""
    lo, hi = 0, len(prefix) - 1
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if prefix[mid] <= w:
            lo = mid
        else:
            hi = mid
    return lo


def chunk_terms(text, run=crc_run):
    """the register of every chunk, each run from state 0"""
    return [run(0, text[chunk_begin(len(text), c):chunk_begin(len(text), c + 1)]) for c in range(chunks_of(len(text)))]


def fold(terms, size):
    """the CRC-32 of a text of `size` bytes from its chunk registers"""
    x = crc_shift(0xFFFFFFFF, size)
    for c, t in enumerate(terms):
        x ^= crc_shift(t, size - chunk_begin(size, c + 1))
    return x ^ 0xFFFFFFFF


def zlib_run(state, data):
    """crc_run through zlib (for long texts): the register, not the finished CRC"""
    return zlib.crc32(data, state ^ 0xFFFFFFFF) ^ 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ what the device answers
def status(data, e, verify=True, cap=1 << 24):
    """(text, SMH_INFLATE_* status) of entry e inflated as the device inflates it; NOT_RUN for an entry it does not take or
    whose announced text is above `cap` (the host program's limit)"""
    if not e.device_ok or e.text_size > cap:
        return b"", NOT_RUN
    src = data[e.payload_off:e.payload_off + e.payload_len]
    if e.kind in (STORED, DIRECTORY):
        text = bytes(src[:e.text_size])
        return text, (IR.CRC if verify and zlib.crc32(text) != e.text_crc else IR.OK)
    return IR.inflate_payload(src, e.text_size, e.text_crc if verify else None)


# ------------------------------------------------------------------------------------------------ a zip written by hand
def raw_deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=-15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(text) + c.flush()


def gz(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, name=b"", extra=b"", comment=b"", hcrc=False, crc=None, isize=None):
    """one gzip member, mtime 0, every optional header field settable"""
    flg = (4 if extra else 0) | (8 if name else 0) | (16 if comment else 0) | (2 if hcrc else 0)
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\x00\xff"
    if extra:
        head += struct.pack("<H", len(extra)) + extra
    if name:
        head += name + b"\0"
    if comment:
        head += comment + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + raw_deflate(text, level, strategy) + struct.pack("<II", zlib.crc32(text) if crc is None else crc,
                                                                   len(text) & 0xFFFFFFFF if isize is None else isize)


def member(name, content, method=0, **kw):
    """a member of build(): content is what the entry holds once the zip layer is undone.  Keys: flags, comp (the bytes as
    stored, instead of compressing content), crc, size, comp_size (the fields, instead of the true values), local_extra,
    central_extra, local_name, descriptor (flag bit 3: zeros in the local header, a descriptor behind the data), zip64 (the
    central sizes and offset go to a zip64 extra field; extra_before: other fields in front of it), level, strategy, comment,
    disk"""
    m = dict(name=name if isinstance(name, bytes) else name.encode(), content=bytes(content), method=method)
    m.update(kw)
    return m


def build(members, comment=b"", zip64_end=False, prepend=b"", eocd_patch=None, cd_cut=0):
    out, central = bytearray(prepend), bytearray()
    for m in members:
        content, method = m["content"], m["method"]
        comp = m.get("comp")
        if comp is None:
            comp = raw_deflate(content, m.get("level", 6), m.get("strategy", zlib.Z_DEFAULT_STRATEGY)) if method == 8 else content
        crc = m.get("crc", zlib.crc32(content))
        size, comp_size = m.get("size", len(content)), m.get("comp_size", len(comp))
        flags = m.get("flags", 0) | (8 if m.get("descriptor") else 0)
        lname, lextra, cextra = m.get("local_name", m["name"]), m.get("local_extra", b""), m.get("central_extra", b"")
        header_off = len(out)
        lcrc, lcs, ls = (0, 0, 0) if m.get("descriptor") else (crc, min(comp_size, 0xFFFFFFFF), min(size, 0xFFFFFFFF))
        out += struct.pack("<4sHHHHHIIIHH", b"PK\3\4", 20, flags, method, 0, 0x21, lcrc, lcs, ls, len(lname), len(lextra)) + lname + lextra
        out += comp
        if m.get("descriptor"):
            out += struct.pack("<4sIII", b"PK\7\x08", crc, comp_size, size)
        c_cs, c_s, c_off = comp_size, size, header_off
        if m.get("zip64"):
            cextra = m.get("extra_before", b"") + struct.pack("<HHQQQ", 1, 24, size, comp_size, header_off) + cextra
            c_cs = c_s = c_off = 0xFFFFFFFF
        ccomment = m.get("comment", b"")
        central += struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\1\2", 20, 20, flags, method, 0, 0x21, crc, c_cs, c_s, len(m["name"]), len(cextra),
                               len(ccomment), m.get("disk", 0), 0, 0, c_off) + m["name"] + cextra + ccomment
    cd_off = len(out)
    if cd_cut:
        central = central[:-cd_cut]
    out += central
    n = len(members)
    if zip64_end:
        z = len(out)
        out += struct.pack("<4sQHHIIQQQQ", b"PK\6\6", 44, 45, 45, 0, 0, n, n, len(central), cd_off)
        out += struct.pack("<4sIQI", b"PK\6\7", 0, z, 1)
        fields = [0, 0, 0xFFFF, 0xFFFF, 0xFFFFFFFF, 0xFFFFFFFF]
    else:
        fields = [0, 0, n, n, len(central), cd_off]
    if eocd_patch:
        for k, v in eocd_patch.items():
            fields[k] = v
    out += struct.pack("<4sHHHHIIH", b"PK\5\6", *fields, len(comment)) + comment
    return bytes(out)


def sig_text(seed, n=40):
    rng = random.Random(seed)
    mins = sorted(rng.sample(range(1 << 40), n))
    return ('[{"class":"sourmash_signature","name":"s%d","signatures":[{"ksize":21,"mins":%s}]}]' % (seed, mins)).replace(" ", "").encode()


def pattern(size, seed):
    """a text with literals, near and far matches"""
    rng = random.Random(seed)
    words = [bytes(rng.choice(b"ACGTN0123456789,") for _ in range(rng.randrange(3, 40))) for _ in range(50)]
    out = bytearray()
    while len(out) < size:
        out += rng.choice(words) if rng.random() < 0.8 else bytes(rng.randrange(256) for _ in range(rng.randrange(1, 30)))
    return bytes(out[:size])


def bad_mix():
    """(archive, the good texts): good members at the even places, a damaged one at every odd place -- a wrong directory
    CRC, a flipped payload byte, a wrong CRC on a stored member, an ISIZE one below the text, a stream cut short"""
    good = [pattern(5000 + i, 300 + i) for i in range(6)]
    t = pattern(40000, 9)
    members = [member("g0.sig.gz", gz(good[0])), member("bad_crc.sig", t, 8, crc=1), member("g1.sig", good[1], 8),
               member("bad_payload.sig", t, 8, comp=_flip(raw_deflate(t), 700)), member("g2.sig", good[2]),
               member("bad_stored.sig", t, crc=2), member("g3.sig.gz", gz(good[3])), member("bad_trailer.sig.gz", gz(t, isize=len(t) - 1)),
               member("g4.sig", good[4], 8), member("short.sig", t, 8, comp=raw_deflate(t)[:-9]), member("g5.sig", good[5])]
    return build(members), good


def host_served():
    """(archive, the four texts a b c d): what the Python layer finishes on the host next to what the device takes -- a .gz of
    two members of different sizes, a plain .gz, a deflated .sig, a .gz deflated once more, a plain .sig and a member that is
    no signature"""
    a, b, c, d = (sig_text(s, 400) for s in (31, 32, 33, 34))
    two = gz(a[:len(a) // 3]) + gz(a[len(a) // 3:])
    members = [member("two.sig.gz", two), member("b.sig.gz", gz(b)), member("c.sig", c, 8), member("double.sig.gz", gz(d), 8),
               member("plain.sig", a), member("notes.txt", b"not a signature")]
    return build(members), (a, b, c, d)


def trailer_and_good():
    """(archive, the two texts): a .gz whose trailer CRC is wrong in front of a good deflated member"""
    b, c = sig_text(32, 400), sig_text(33, 400)
    return build([member("bad.sig.gz", gz(b, crc=3)), member("c.sig", c, 8)]), (b, c)


def equal_halves():
    """(archive, one half): a .gz of two members of the SAME size -- ISIZE fits the first one, so the device reports the bytes
    left over behind it"""
    half = pattern(4000, 8)
    return build([member("eq.sig.gz", gz(half) + gz(half))]), half


def three():
    """a small valid archive: a stored .sig.gz, a deflated .sig and a plain stored .sig"""
    return build([member("signatures/a.sig.gz", gz(sig_text(1))), member("b.sig", sig_text(2), 8), member("c.sig", sig_text(3))])


def crafted():
    """[(name, archive bytes)]: valid archives of every shape and one archive per refusal"""
    a, b, c = gz(sig_text(1)), sig_text(2), sig_text(3)
    base = [member("signatures/a.sig.gz", a), member("b.sig", b, 8), member("c.sig", c)]
    fake_end = b"xx" + struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, 0, 0, 0, 0, 0)      # a consistent empty end record, in the comment
    out = [
        ("three", build(base)),
        ("empty", build([])),
        ("empty_zip64", build([], zip64_end=True)),
        ("directories", build([member("signatures/", b""), member("signatures/a.sig.gz", a), member("d/", b"", 8, comp=b"\x03\x00")])),
        ("not_a_directory", build([member("odd/", b"xy")])),
        ("descriptor", build([member("a.sig.gz", a, descriptor=True), member("b.sig", b, 8, descriptor=True)])),
        ("local_extra_longer", build([member("a.sig.gz", a, local_extra=b"\x55\x55\x08\0" + b"q" * 8, central_extra=b""),
                                      member("b.sig", b, 8, local_extra=b"\x99\x99\x01\0z")])),
        ("local_name_longer", build([member("b.sig", b, 8, local_name=b"another-name.sig"), member("c.sig", c, local_name=b"")])),
        ("comment_plain", build(base, comment=b"a comment")),
        ("comment_with_signature", build(base, comment=b"see PK\5\6 and PK\5\6\0\0 for details")),
        ("comment_with_end_record", build(base, comment=fake_end)),
        ("zip64_end", build(base, zip64_end=True)),
        ("zip64_extra", build([member("a.sig.gz", a, zip64=True), member("b.sig", b, 8, zip64=True, central_extra=b"\x77\x77\x02\0ab")])),
        ("zip64_extra_behind_another", build([member("b.sig", b, 8, zip64=True, extra_before=b"\x0a\x00\x03\x00abc")])),
        ("entry_comment", build([member("a.sig.gz", a, comment=b"hello"), member("c.sig", c)])),
        ("gzip_fields", build([member("g%d.sig.gz" % k, gz(sig_text(10 + k), name=b"n" * k, comment=b"c" * (k % 3), hcrc=bool(k & 1),
                                                         extra=(b"AB" + struct.pack("<H", k) + b"e" * k) if k % 2 else b"")) for k in range(6)])),
        ("gzip_short", build([member("s.sig.gz", b"\x1f\x8b\x08\x00\0\0\0\0\x00\xff\x03\x00\0\0\0")])),
        ("gzip_header_cut", build([member("s.sig.gz", b"\x1f\x8b\x08\x08\0\0\0\0\x00\xff" + b"name-without-nul" * 2)])),
        ("gzip_two_members", build([member("two.sig.gz", gz(sig_text(4)) + gz(sig_text(5)))])),
        ("encrypted", build([member("e.sig", c, flags=1), member("c.sig", c)])),
        ("method_12", build([member("bz.sig", c, 12), member("c.sig", c)])),
        ("stored_sizes_differ", build([member("c.sig", c, size=len(c) + 1)])),
        ("size_2_32", build([member("big.sig", b"", 8, comp=b"\x03\x00", zip64=True, size=1 << 32)])),
        ("wrong_crc", build([member("c.sig", c, crc=zlib.crc32(c) ^ 1), member("b.sig", b, 8, crc=5)])),
        ("wrong_trailer", build([member("a.sig.gz", gz(sig_text(1), crc=7))])),
        ("flipped_payload", build([member("b.sig", b, 8, comp=_flip(raw_deflate(b), 9))])),
        ("doubly_compressed", build([member("a.sig.gz", a, 8)])),
        ("reserved_block", build([member("r.sig", c, 8, comp=b"\x07\x00"), member("c.sig", c)])),
        ("bad_mix", bad_mix()[0]),
        ("host_served", host_served()[0]),
        ("trailer_and_good", trailer_and_good()[0]),
        ("equal_halves", equal_halves()[0]),
        # refusals
        ("no_end", build(base)[:-1]),
        ("nothing", b""),
        ("multi_disk_end", build(base, eocd_patch={0: 1})),
        ("multi_disk_counts", build(base, eocd_patch={2: 2})),
        ("multi_disk_entry", build([member("c.sig", c, disk=1)])),
        ("cd_outside", build(base, eocd_patch={5: 1 << 20})),
        ("cd_truncated_count", build(base, eocd_patch={2: 4, 3: 4})),
        ("cd_truncated_size", build(base, eocd_patch={4: 50})),
        ("cd_signature", build(base).replace(b"PK\1\2", b"PK\1\3", 1)),
        ("local_signature", build(base).replace(b"PK\3\4", b"PK\3\5", 1)),
        ("zip64_extra_missing", build([member("c.sig", c, zip64=True)]).replace(b"\x01\x00\x18\x00", b"\x02\x00\x18\x00", 1)),
        ("zip64_extra_short", build([member("c.sig", c, zip64=True)]).replace(b"\x01\x00\x18\x00", b"\x01\x00\x10\x00", 1)),
        ("zip64_end_outside", _patch_locator(build(base, zip64_end=True), 1 << 40)),
        ("data_outside", build([member("c.sig", c, comp_size=len(c) + 4096, size=len(c) + 4096)])),
    ]
    hdr = build([member("c.sig", c)])
    at = hdr.index(b"PK\1\2") + 42
    out.append(("local_outside", hdr[:at] + struct.pack("<I", len(hdr) - 10) + hdr[at + 4:]))
    return out


def _flip(data, at):
    return data[:at] + bytes([data[at] ^ 0x20]) + data[at + 1:]


def _patch_locator(data, z):
    at = data.rindex(b"PK\6\7") + 8
    return data[:at] + struct.pack("<Q", z) + data[at + 8:]


REFUSALS = {"no_end": "no end-of-central-directory record", "nothing": "no end-of-central-directory record",
            "multi_disk_end": "multi-disk archive", "multi_disk_counts": "multi-disk archive", "multi_disk_entry": "multi-disk archive",
            "cd_outside": "central directory outside the data", "cd_truncated_count": "truncated central directory",
            "cd_truncated_size": "truncated central directory", "cd_signature": "central directory entry without its signature",
            "local_signature": "local header without its signature", "zip64_extra_missing": "zip64 extra field missing or cut short",
            "zip64_extra_short": "zip64 extra field missing or cut short",
            "zip64_end_outside": "zip64 end record outside the data or without its signature", "data_outside": "entry data outside the data",
            "local_outside": "local header outside the data"}


def mutants(n=2000, seed=29):
    """byte-level mutants of the small valid archive: one to three bytes replaced, and some truncated or extended"""
    rng = random.Random(seed)
    base = three()
    hot = [i for i in range(len(base)) if base[i:i + 2] == b"PK"]          # half of the mutations land in a header
    out = []
    for k in range(n):
        d = bytearray(base)
        for _ in range(rng.randrange(1, 4)):
            if rng.random() < 0.5:
                at = min(len(d) - 1, rng.choice(hot) + rng.randrange(0, 46))
            else:
                at = rng.randrange(len(d))
            d[at] = rng.choice((0, 1, 0xFF, d[at] ^ (1 << rng.randrange(8)), rng.randrange(256)))
        if k % 17 == 0:
            d = d[:rng.randrange(len(d))]
        elif k % 19 == 0:
            d += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 40)))
        out.append(bytes(d))
    return out
