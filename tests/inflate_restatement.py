"""Blocked gzip in plain Python: the member scan and the DEFLATE rules of include/sourmash_amd.h ("Blocked gzip"), stated
once more without the library, plus the fixtures the inflate tests share (a BGZF writer on zlib, a bit writer for hand-made
blocks, the crafted valid and malformed members and the seeded fuzz).

    scan(data)                     -> [Member]; ScanError(index, offset, what) on a refusal
    inflate_raw(payload, cap)      -> (bytes, reason): the first rule the stream breaks, 0 for none
    inflate_member(data, member, verify) -> (bytes, reason): with ISIZE and the CRC-32 checked

The decoder reads a symbol one bit at a time down the canonical code, so "input exhausted" and "no such code" are decided the
same way everywhere.  It is pinned to zlib by tests/test_inflate_rules.py."""
import random
import struct
import zlib
from collections import namedtuple

OK, BLOCK_TYPE, STORED_LEN, HEADER_COUNTS, REPEAT, OVER, INCOMPLETE, NO_EOB, BAD_SYMBOL, DISTANCE, INPUT, OUT_OVER, OUT_UNDER, \
    LEFTOVER, CRC = range(15)
MAX_MEMBER = 65536

Member = namedtuple("Member", "header_off payload_off payload_len isize crc out_off")


class ScanError(Exception):
    def __init__(self, index, offset, what):
        Exception.__init__(self, "%s (member %d at byte %d)" % (what, index, offset))
        self.index, self.offset, self.what = index, offset, what


# ---------------------------------------------------------------------------------------------------------------- scan
def scan(data):
    data = bytes(data)
    members, off, out = [], 0, 0
    while off < len(data):
        index, h = len(members), data[off:]
        left = len(h)
        magic = h[:2] == b"\x1f\x8b" if left >= 2 else h[0] == 0x1f
        if not magic or (left >= 3 and h[2] != 8):
            raise ScanError(index, off, "not gzip" if index == 0 else "bytes trail after the last member")
        cut = ScanError(index, off, "header is cut short")
        if left < 10:
            raise cut
        flg, at, bsize = h[3], 10, None
        if flg & 4:
            if left < at + 2:
                raise cut
            xlen = h[at] | h[at + 1] << 8
            at += 2
            if left < at + xlen:
                raise cut
            sub, end = at, at + xlen
            while sub < end:
                if end - sub < 4:
                    raise cut
                slen = h[sub + 2] | h[sub + 3] << 8
                if end - sub - 4 < slen:
                    raise cut
                if h[sub:sub + 2] == b"BC" and slen == 2 and bsize is None:
                    bsize = h[sub + 4] | h[sub + 5] << 8
                sub += 4 + slen
            at = end
        for bit in (8, 16):
            if flg & bit:
                nul = h.find(b"\0", at)
                if nul < 0:
                    raise cut
                at = nul + 1
        if flg & 2:
            at += 2
        if at > left:
            raise cut
        if bsize is None:
            raise ScanError(index, off, "not blocked gzip")
        total = bsize + 1
        if total > left:
            raise ScanError(index, off, "BSIZE runs past the end")
        if at + 8 > total:
            raise cut
        crc, isize = struct.unpack("<II", h[total - 8:total])
        if isize > MAX_MEMBER:
            raise ScanError(index, off, "ISIZE above 65536")
        members.append(Member(off, off + at, total - at - 8, isize, crc, out))
        out += isize
        off += total
    return members


# ------------------------------------------------------------------------------------------------------------- inflate
class _Bits:
    def __init__(self, data):
        self.d, self.bit = data, 0                     # bit: the next bit, counted from the payload's start

    def left(self):
        return len(self.d) * 8 - self.bit

    def take(self, n):                                  # None: fewer than n bits are left (nothing is consumed)
        if self.left() < n:
            return None
        v = 0
        for i in range(n):
            p = self.bit + i
            v |= (self.d[p >> 3] >> (p & 7) & 1) << i
        self.bit += n
        return v


def _build(lens):
    """(count per length, symbols by (length, symbol), 0 built / 1 over-subscribed / 2 incomplete, coded symbols)"""
    cnt = [0] * 16
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    left, over = 1, False
    for l in range(1, 16):
        left = (left << 1) - cnt[l]
        if left < 0:
            over, left = True, 0
    sym = [s for l in range(1, 16) for s, sl in enumerate(lens) if sl == l]
    return cnt, sym, (1 if over else 2 if left > 0 else 0), len(sym)


def _decode(b, cnt, sym):
    """a symbol; -1: input exhausted; -2: no code matches"""
    code = first = index = 0
    have = min(b.left(), 15)
    for l in range(1, 16):
        if l > have:
            return -1
        p = b.bit + l - 1
        code |= b.d[p >> 3] >> (p & 7) & 1
        if code < first + cnt[l]:
            b.bit += l
            return sym[index + code - first]
        index += cnt[l]
        first = (first + cnt[l]) << 1
        code <<= 1
    return -2


_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
          12289, 16385, 24577)
_DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
_FIXED = None


def _dynamic(b):
    if b.left() < 14:
        return INPUT, None, None
    nlen, ndist, ncode = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    if nlen > 286 or ndist > 30:
        return HEADER_COUNTS, None, None
    clens = [0] * 19
    for i in range(ncode):
        v = b.take(3)
        if v is None:
            return INPUT, None, None
        clens[_ORDER[i]] = v
    ccnt, csym, r, _ = _build(clens)
    if r:
        return (OVER if r == 1 else INCOMPLETE), None, None
    total, lens = nlen + ndist, []
    while len(lens) < total:
        s = _decode(b, ccnt, csym)
        if s == -1:
            return INPUT, None, None
        if s < 0:
            return BAD_SYMBOL, None, None
        if s < 16:
            lens.append(s)
            continue
        val = 0
        if s == 16:
            if not lens:
                return REPEAT, None, None
            e = b.take(2)
            if e is None:
                return INPUT, None, None
            val, rep = lens[-1], 3 + e
        elif s == 17:
            e = b.take(3)
            if e is None:
                return INPUT, None, None
            rep = 3 + e
        else:
            e = b.take(7)
            if e is None:
                return INPUT, None, None
            rep = 11 + e
        if rep > total - len(lens):
            return REPEAT, None, None
        lens += [val] * rep
    if lens[256] == 0:
        return NO_EOB, None, None
    lcnt, lsym, r, coded = _build(lens[:nlen])
    if r == 1:
        return OVER, None, None
    if r == 2 and not (coded == 1 and lcnt[1] == 1):
        return INCOMPLETE, None, None
    dcnt, dsym, r, coded = _build(lens[nlen:])
    if r == 1:
        return OVER, None, None
    if r == 2 and not (coded == 0 or (coded == 1 and dcnt[1] == 1)):
        return INCOMPLETE, None, None
    return OK, (lcnt, lsym), (dcnt, dsym)


def inflate_raw(payload, cap=MAX_MEMBER):
    """(bytes, reason): at most `cap` bytes; OUT_OVER when the stream would write more."""
    global _FIXED
    payload = bytes(payload)
    b, out = _Bits(payload), bytearray()
    while True:
        if b.left() < 3:
            return bytes(out), INPUT
        last, kind = b.take(1), b.take(2)
        if kind == 3:
            return bytes(out), BLOCK_TYPE
        if kind == 0:
            pos = (b.bit + 7) >> 3
            if len(payload) - pos < 4:
                return bytes(out), INPUT
            n, nn = struct.unpack("<HH", payload[pos:pos + 4])
            pos += 4
            if n != nn ^ 0xffff:
                return bytes(out), STORED_LEN
            if n > len(payload) - pos:
                return bytes(out), INPUT
            if n > cap - len(out):
                return bytes(out), OUT_OVER
            out += payload[pos:pos + n]
            b.bit = (pos + n) * 8
        else:
            if kind == 1:
                if _FIXED is None:
                    l = _build([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
                    d = _build([5] * 32)
                    _FIXED = (l[0], l[1]), (d[0], d[1])
                lit, dis = _FIXED
            else:
                r, lit, dis = _dynamic(b)
                if r:
                    return bytes(out), r
            while True:
                s = _decode(b, *lit)
                if s == -1:
                    return bytes(out), INPUT
                if s < 0:
                    return bytes(out), BAD_SYMBOL
                if s < 256:
                    if len(out) >= cap:
                        return bytes(out), OUT_OVER
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    return bytes(out), BAD_SYMBOL
                e = b.take(_LEXT[s - 257])
                if e is None:
                    return bytes(out), INPUT
                length = _LBASE[s - 257] + e
                ds = _decode(b, *dis)
                if ds == -1:
                    return bytes(out), INPUT
                if ds < 0 or ds > 29:
                    return bytes(out), BAD_SYMBOL
                e = b.take(_DEXT[ds])
                if e is None:
                    return bytes(out), INPUT
                dist = _DBASE[ds] + e
                if dist > len(out):
                    return bytes(out), DISTANCE
                if length > cap - len(out):
                    return bytes(out), OUT_OVER
                for _ in range(length):
                    out.append(out[-dist])
        if last:
            break
    return bytes(out), (b.bit, len(payload))


def _finish(out, tail, isize):
    """the checks behind the final block: tail = (bits consumed, payload bytes) or a reason"""
    if not isinstance(tail, tuple):
        return tail
    if len(out) < isize:
        return OUT_UNDER
    if (tail[0] + 7) >> 3 < tail[1]:
        return LEFTOVER
    return OK


def inflate_payload(payload, isize, crc=None):
    """one member's payload against its trailer: (bytes, reason); crc None: not verified"""
    out, tail = inflate_raw(payload, isize)
    r = _finish(out, tail, isize)
    if r == OK and crc is not None and zlib.crc32(out) != crc:
        r = CRC
    return out, r


def inflate_member(data, m, verify=True):
    return inflate_payload(data[m.payload_off:m.payload_off + m.payload_len], m.isize, m.crc if verify else None)


def inflate_stream(payload):
    """a payload on its own, as zlib.decompressobj(-15) sees it: (bytes, reason) with the output capped at 65 536"""
    out, tail = inflate_raw(payload, MAX_MEMBER)
    return out, _finish(out, tail, len(out))


# ------------------------------------------------------------------------------------------------------------ fixtures
def member(payload, text_or_isize, crc=None, name=None, comment=None, extra_before=b"", extra_after=b"", hcrc=False):
    """one BGZF member around a raw DEFLATE payload; text_or_isize: the text (ISIZE and CRC from it) or an ISIZE"""
    if isinstance(text_or_isize, int):
        isize, crc = text_or_isize, (crc or 0)
    else:
        isize, crc = len(text_or_isize), (zlib.crc32(text_or_isize) if crc is None else crc)
    flg = 4 | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    opt = b"".join(x + b"\0" for x in (name, comment) if x is not None) + (b"\x12\x34" if hcrc else b"")
    xlen = len(extra_before) + 6 + len(extra_after)
    total = 12 + xlen + len(opt) + len(payload) + 8
    assert total <= 65536
    extra = extra_before + b"BC" + struct.pack("<HH", 2, total - 1) + extra_after
    return b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + opt + payload + \
        struct.pack("<II", crc & 0xffffffff, isize)


def subfield(tag, n):
    return tag + struct.pack("<H", n) + bytes(range(n))


def deflate(text, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, flush_mode=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    if not flush_every:
        return c.compress(text) + c.flush()
    out = b""
    for i in range(0, len(text), flush_every):
        out += c.compress(text[i:i + flush_every]) + c.flush(flush_mode)
    return out + c.flush()


EOF_MEMBER = member(b"\x03\x00", b"")


def bgzf(text, block=65280, level=6, eof=True):
    text = bytes(text)
    return b"".join(member(deflate(text[i:i + block], level), text[i:i + block]) for i in range(0, len(text), block)) + \
        (EOF_MEMBER if eof else b"")


class BitWriter:
    """LSB-first bits; Huffman codes go in most significant bit first"""

    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits += [(value >> i) & 1 for i in range(n)]
        return self

    def code(self, value, n):
        self.bits += [(value >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def fixed_lit(self, s):
        if s < 144:
            return self.code(0x30 + s, 8)
        if s < 256:
            return self.code(0x190 + s - 144, 9)
        if s < 280:
            return self.code(s - 256, 7)
        return self.code(0xc0 + s - 280, 8)

    def fixed_match(self, length, dist):
        ls = max(i for i in range(29) if _LBASE[i] <= length and (i == 28 or length < 258))
        self.fixed_lit(257 + ls).put(length - _LBASE[ls], _LEXT[ls])
        ds = max(i for i in range(30) if _DBASE[i] <= dist)
        return self.code(ds, 5).put(dist - _DBASE[ds], _DEXT[ds])

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + j] << j for j in range(8)) for i in range(0, len(b), 8))


def fastq_text(reads=100, bases=150, seed=1):
    rng = random.Random(seed)
    out = []
    for i in range(reads):
        out.append(b"@read%d\n%s\n+\n%s\n" % (i, bytes(rng.choice(b"ACGT") for _ in range(bases)),
                                              bytes(rng.choice(b"FFFFF:,#") for _ in range(bases))))
    return b"".join(out)


def fibonacci_text():
    """bytes whose frequencies are Fibonacci numbers, shuffled: Z_HUFFMAN_ONLY gives them code lengths up to 15"""
    fib, text = [1, 1], bytearray()
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    for i, f in enumerate(fib):
        text += bytes([65 + i]) * f
    random.Random(5).shuffle(text)
    return bytes(text)


def dynamic_header(nlen, ndist, clens, symbols):
    """BFINAL=1 dynamic block header: clens = the 19 code-length-code lengths by symbol; symbols = [(code, bits, extra,
    extra_bits)] written as they are"""
    w = BitWriter().put(1, 1).put(2, 2).put(nlen - 257, 5).put(ndist - 1, 5)
    ncode = max(4, max(i for i in range(19) if clens[_ORDER[i]] or i < 4) + 1)
    w.put(ncode - 4, 4)
    for i in range(ncode):
        w.put(clens[_ORDER[i]], 3)
    for code, n, extra, en in symbols:
        w.code(code, n).put(extra, en)
    return w


def valid_cases():
    """[(name, payload, text)]: every one decodes under zlib"""
    fq = fastq_text()
    rng = random.Random(11)
    cases = [("stored", deflate(fq, 0), fq),
             ("fixed", deflate(fq, 6, 8, zlib.Z_FIXED), fq),
             ("dynamic", deflate(fq), fq),
             ("memlevel1", deflate(fq, 6, 1), fq),
             ("sync_flush", deflate(fq, 6, 8, flush_every=1000), fq),
             ("full_flush", deflate(fq, 6, 8, flush_every=1000, flush_mode=zlib.Z_FULL_FLUSH), fq),
             ("huffman_only", deflate(fq, 6, 8, zlib.Z_HUFFMAN_ONLY), fq),
             ("fibonacci", deflate(fibonacci_text(), 6, 8, zlib.Z_HUFFMAN_ONLY), fibonacci_text()),
             ("run_a", deflate(b"A" * 65280), b"A" * 65280),
             ("run_ab", deflate(b"AB" * 2000), b"AB" * 2000)]
    half = bytes(rng.choice(b"ACGT") for _ in range(32500))
    cases.append(("far_repeat", deflate(half * 2, 9), half * 2))
    lits = bytes(rng.randrange(144) for _ in range(32768))
    w = BitWriter().put(1, 1).put(1, 2)
    text = bytearray(lits)
    for s in lits:
        w.fixed_lit(s)
    for length, dist in ((258, 32768), (3, 1), (258, 1), (4, 32768)):
        w.fixed_match(length, dist)
        for _ in range(length):
            text.append(text[-dist])
    cases.append(("max_distance", w.fixed_lit(256).bytes(), bytes(text)))
    for n in (0, 1, 63, 64, 65, 65280, 65535, 65536):
        t = bytes(rng.choice(b"ACGTN\n") for _ in range(n))
        cases.append(("size_%d" % n, deflate(t), t))
    noise = bytes(rng.randrange(256) for _ in range(3000))
    cases.append(("noise", deflate(noise, 6, 8, zlib.Z_FIXED), noise))
    # a literal/length set of one single 1-bit code (the end of the block) and no distance code at all: legal
    cases.append(("single_code", dynamic_header(257, 1, _single_clens(), _single_symbols()).bytes(), b""))
    return cases


def _single_clens():
    c = [0] * 19
    c[0], c[1], c[18] = 2, 2, 1      # complete: 18 -> '0', 0 -> '10', 1 -> '11'
    return c


def _single_symbols():
    # 256 zeros (138 + 118), length 1 for symbol 256, length 0 for the one distance code
    return [(0, 1, 127, 7), (0, 1, 107, 7), (3, 2, 0, 0), (2, 2, 0, 0), (0, 1, 0, 0)]


def malformed_cases():
    """[(name, payload, isize, reason)]: zlib rejects every one but the ISIZE and leftover ones, which it cannot see"""
    fq = fastq_text()
    good = deflate(fq)
    cases = [("block_type_3", BitWriter().put(1, 1).put(3, 2).bytes(), 0, BLOCK_TYPE),
             ("stored_nlen", b"\x01\x05\x00\xfb\xff" + b"hello", 5, STORED_LEN),
             ("symbol_286", BitWriter().put(1, 1).put(1, 2).fixed_lit(65).fixed_lit(286).put(0, 16).bytes(), 100, BAD_SYMBOL),
             ("distance_30", BitWriter().put(1, 1).put(1, 2).fixed_lit(65).fixed_lit(257).code(30, 5).put(0, 16).bytes(), 100, BAD_SYMBOL),
             ("match_at_0", BitWriter().put(1, 1).put(1, 2).fixed_match(3, 1).fixed_lit(256).bytes(), 3, DISTANCE),
             ("distance_2_at_1", BitWriter().put(1, 1).put(1, 2).fixed_lit(65).fixed_match(3, 2).fixed_lit(256).bytes(), 4, DISTANCE),
             ("cut_mid_symbol", good[:len(good) // 2], len(fq), INPUT)]
    over = [0] * 19
    over[0], over[1], over[2] = 1, 1, 1
    cases.append(("over_subscribed", dynamic_header(257, 1, over, []).put(0, 32).bytes(), 0, OVER))
    inc = [0] * 19
    inc[0], inc[1] = 1, 2
    cases.append(("incomplete", dynamic_header(257, 1, inc, []).put(0, 32).bytes(), 0, INCOMPLETE))
    cases.append(("hlit_287", BitWriter().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(0, 4).put(0, 32).bytes(), 0, HEADER_COUNTS))
    cases.append(("leading_repeat", dynamic_header(257, 1, _repeat_clens(), [(1, 1, 0, 2)]).put(0, 32).bytes(), 0, REPEAT))
    cases.append(("one_over", good, len(fq) - 1, OUT_OVER))
    cases.append(("one_under", good, len(fq) + 1, OUT_UNDER))
    cases.append(("leftover", good + b"\0", len(fq), LEFTOVER))
    return cases


def _repeat_clens():
    c = [0] * 19
    c[16], c[0] = 1, 1               # 0 -> '0', 16 -> '1' in canonical order (symbol 0 first)
    return c


def fuzz_mutants(n=2000, seed=23):
    """[(payload, isize, crc)]: single- and double-bit flips of valid payloads of at most 2 KiB; ISIZE and CRC are the
    original text's"""
    rng = random.Random(seed)
    fq = fastq_text(12, 60, 3)
    seeds = [(deflate(fq), fq), (deflate(fq, 6, 8, zlib.Z_FIXED), fq), (deflate(fq[:300], 0), fq[:300]),
             (deflate(fq, 6, 1), fq), (deflate(fq, 6, 8, flush_every=500), fq), (deflate(b"AB" * 900), b"AB" * 900)]
    assert all(len(p) <= 2048 for p, _ in seeds)
    out = []
    for i in range(n):
        p, t = seeds[i % len(seeds)]
        p = bytearray(p)
        for _ in range(1 + (i // len(seeds)) % 2):
            k = rng.randrange(len(p) * 8)
            p[k >> 3] ^= 1 << (k & 7)
        out.append((bytes(p), len(t), zlib.crc32(t)))
    return out
