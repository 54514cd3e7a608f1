"""The device parser (fastx.Records, C ABI smh_records_*) against the format rules restated in tests/fastx_restatement.py:
offsets, the compacted bytes and the name spans, over the literals of the contract, every kind of line structure placed
on the boundaries of the parser's tiles, every alignment of the text pointer, the error reports, sketches built from the
parsed records against sketches of records cut on the host, gzip input, and a text past 4 GiB."""
import gzip
import random
import re

import numpy as np
import pytest
import torch

import fastx_restatement as R

pytestmark = pytest.mark.gpu

FASTA_LIT = b"\n\r\n>a\r\nAC\r\nGT\n\n>b\n>c d\nA>C\rG\r"
FASTQ_LIT = b"@r1\nACGT\n+\n@@@@\n@r2 x\r\nAC\r\n+r2 x\r\n+>\r\n\n\n"


@pytest.fixture(scope="module")
def T(pkg):
    return pkg.lib().smh_records_tile_bytes()


def dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def device_text(text, lead=0):
    """The text as a CUDA uint8 view that starts `lead` bytes into its tensor."""
    buf = torch.full((lead + len(text) + 16,), 0x3E, dtype=torch.uint8)    # '>' all around: a read outside the view shows
    buf[lead:lead + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8) if text else buf[0:0]
    return buf.cuda()[lead:lead + len(text)]


def check(pkg, text, fmt="auto", device=False, lead=0):
    """parse `text` and compare the three things with the restatement; returns the Records."""
    want_fmt, recs, spans = R.parse(text, fmt)
    got = pkg.Records.parse(device_text(text, lead) if device else text, fmt)
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs], dtype=np.uint64)
    assert got.format == want_fmt
    assert len(got) == len(recs) and got.total == int(off[-1])
    assert np.array_equal(got.offsets, off)
    assert bytes(got.seq_tensor().cpu().numpy()) == b"".join(recs)
    start, length = got.name_spans()
    assert [(int(s), int(n)) for s, n in zip(start, length)] == spans
    assert got.names(text) == [text[s:s + n] for s, n in spans]
    return got


def parse_error(pkg, text, fmt="auto", device=False):
    with pytest.raises(pkg.SourmashError) as ei:
        pkg.Records.parse(device_text(text) if device else text, fmt)
    assert ei.value.code == 3
    return ei.value.message


# ---------------------------------------------------------------------------------------------------------------- 1

@pytest.mark.parametrize("device", [False, True])
def test_literals(pkg, device):
    for fmt in ("auto", "fasta"):
        check(pkg, FASTA_LIT, fmt, device)
        check(pkg, b">a", fmt, device)
    for fmt in ("auto", "fastq"):
        check(pkg, FASTQ_LIT, fmt, device)
        check(pkg, b"@e\n\n+\n\n", fmt, device)
        check(pkg, b"@e\n\n+", fmt, device)
    for fmt in ("auto", "fasta", "fastq"):
        r = check(pkg, b"", fmt, device)
        assert len(r) == 0 and r.total == 0
    check(pkg, b"\n\r\n\n", "fasta", device)
    check(pkg, b"\n\n", "fastq", device)
    # a wrong explicit format is an error, and so is a text that is neither
    assert "byte 3" in parse_error(pkg, b"\n\r\n" + FASTQ_LIT, "fasta", device)
    assert "record 0" in parse_error(pkg, FASTA_LIT, "fastq", device)
    parse_error(pkg, b"\nACGT\n", "auto", device)
    for text, rec in [(b"@a\nACGT\n+\nIII\n", 0), (b"a\nACGT\n+\nIIII\n", 0), (b"@a\nACGT\n-\nIIII\n", 0),
                      (b"@a\nACGT\n+\nIIII\n@b\nAC\n+\n", 1)]:
        assert "record %d" % rec in parse_error(pkg, text, "fastq", device)
    assert "byte 0" in parse_error(pkg, b"AC\n>a\n", "fasta", device)


# ---------------------------------------------------------------------------------------------------------------- 2

def boundary_positions(T):
    return [T - 2, T - 1, T, T + 1, 2 * T - 2, 2 * T - 1, 2 * T, 2 * T + 1]


def filler(rng, p):
    """p bytes of FASTA that end a line: one record whose sequence line reaches byte p - 1."""
    return b">f\n" + dna(rng, p - 4) + b"\n"


def test_fasta_tile_boundaries(pkg, T):
    rng = random.Random(2)
    for p in boundary_positions(T):
        tail = b">hdr " + dna(rng, 5) + b"\n" + dna(rng, 37) + b"\n" + dna(rng, 11) + b"\n>z\n" + dna(rng, 9)
        check(pkg, filler(rng, p) + tail, "fasta", True)                                        # a header starts at p
        check(pkg, b">f\n" + dna(rng, p - 3) + b"\r\n" + dna(rng, 21) + b"\r\n>z\r\n" + dna(rng, 5), "fasta", True)   # '\r' at p, '\n' at p + 1
        check(pkg, b">f\r\n" + dna(rng, p - 4) + b"\r" + dna(rng, 7) + b"\n", "fasta", True)     # a '\r' at p that is NOT a terminator
        check(pkg, filler(rng, p) + b"\n" + dna(rng, 21) + b"\n", "fasta", True)                 # an empty line at p
        check(pkg, b">f\n" + dna(rng, p - 3) + b">" + dna(rng, 21) + b"\n", "fasta", True)       # '>' in mid-line at p
        check(pkg, filler(rng, p), "fasta", True)                                                # the text ends at p, with '\n'
        check(pkg, b">f\n" + dna(rng, p - 3), "fasta", True)                                     # ... and without
        check(pkg, b">f\n" + dna(rng, p - 4) + b"\r", "fasta", True)                             # ... and on a '\r'
        check(pkg, filler(rng, p - 3) + b">ab", "fasta", True)                                   # ... and inside a header
        check(pkg, filler(rng, p) + tail, "fasta", False)                                        # host text: uploaded first


def test_fasta_long_lines(pkg, T):
    rng = random.Random(3)
    check(pkg, b">a\n" + dna(rng, 3 * T + 5) + b"\n>b\n" + dna(rng, 10) + b"\n", "fasta", True)
    check(pkg, b">" + dna(rng, 2 * T + 2, b"hdr xyz") + b"\n" + dna(rng, 50) + b"\n>b\r\n" + dna(rng, 10), "fasta", True)
    # tiles without any line start, entered on a header and left on a sequence line
    check(pkg, b">" + dna(rng, 3 * T, b"h>") + b"\r\n" + dna(rng, 4 * T + 1) + b"\r\n>c\n", "fasta", True)


@pytest.mark.parametrize("width", [1, 60, 61, 80])
def test_fasta_wrap_widths(pkg, T, width):
    rng = random.Random(width)
    parts = []
    for i, n in enumerate([0, 1, width, width + 1, 5 * width - 1, T // 2 + 7, T + 13, 3, 2 * T // 3]):
        seq = dna(rng, n, b"ACGTNacgt")
        eol = b"\r\n" if i % 3 == 2 else b"\n"
        parts.append(b">rec%d some words" % i + eol)
        parts.extend(seq[j:j + width] + eol for j in range(0, n, width))
    check(pkg, b"".join(parts), "auto", True)


# ---------------------------------------------------------------------------------------------------------------- 3

def fastq_records(rng, n, read=150):
    """[(name, sequence, plus, quality)]; every quality line begins with '@'."""
    out = []
    for i in range(n):
        seq = dna(rng, read, b"ACGT" * 10 + b"N")
        out.append((b"r%d/1" % i, seq, b"" if i % 2 else b"r%d/1" % i, b"@" + dna(rng, read - 1, b"@+>I#5F")))
    return out


def fastq_text(recs, eol=b"\n", last_eol=True):
    text = b"".join(b"@" + n + eol + s + eol + b"+" + p + eol + q + eol for n, s, p, q in recs)
    return text if last_eol else text[:len(text) - len(eol)]


def line_start(recs, eol, k, which):
    """byte at which line `which` of record k starts"""
    at = len(fastq_text(recs[:k], eol))
    n, s, p, q = recs[k]
    for ln in (b"@" + n, s, b"+" + p, q)[:which]:
        at += len(ln) + len(eol)
    return at


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
def test_fastq_tile_boundaries(pkg, T, eol):
    rng = random.Random(4)
    base = fastq_records(rng, 3 * T // 300)
    for which in range(4):
        for target in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
            k = max(i for i in range(len(base)) if line_start(base, eol, i, which) <= target)
            recs = list(base)
            recs[0] = (base[0][0] + b"x" * (target - line_start(base, eol, k, which)),) + base[0][1:]
            assert line_start(recs, eol, k, which) == target
            if which == 3:
                assert recs[k][3][:1] == b"@"             # a quality line that begins with '@' on the tile's first bytes
            check(pkg, fastq_text(recs, eol), "auto", True)
    check(pkg, fastq_text(base, eol, last_eol=False), "fastq", True)
    check(pkg, fastq_text(base, eol) + eol * 3, "fastq", False)


# ---------------------------------------------------------------------------------------------------------------- 4

def test_alignment(pkg, T):
    rng = random.Random(5)
    parts = []
    for i in range(40):
        parts.append(b">s%d\n" % i)
        seq = dna(rng, rng.randrange(0, 700))
        parts.extend(seq[j:j + 60] + b"\n" for j in range(0, len(seq), 60))
    text = b"".join(parts)
    assert len(text) > 2 * T + 64
    m = (2 * T + 32) // 16
    for lead in range(1, 16):
        check(pkg, text[:16 * m + lead], "fasta", True, lead)
        check(pkg, text[:16 * m + 16 - lead], "fasta", True, lead)
    for lead in (1, 8, 15):
        check(pkg, text[:T - lead], "fasta", True, lead)              # the view ends on a tile boundary of the address
        check(pkg, text[:T - lead + 1], "fasta", True, lead)
        check(pkg, fastq_text(fastq_records(rng, 2 * T // 300)), "fastq", True, lead)


# ---------------------------------------------------------------------------------------------------------------- 5

def break_record(recs, k, kind):
    n, s, p, q = recs[k]
    out = list(recs)
    if kind == "no_at":
        return fastq_text(out[:k]) + b"X" + fastq_text(out[k:])[1:]
    if kind == "no_plus":
        return fastq_text(recs[:k]) + b"@" + n + b"\n" + s + b"\n-" + p + b"\n" + q + b"\n" + fastq_text(recs[k + 1:])
    if kind == "qual_short":
        out[k] = (n, s, p, q[:-1])
    elif kind == "qual_long":
        out[k] = (n, s, p, q + b"I")
    elif kind == "seq_empty":
        out[k] = (n, b"", p, q)
    if kind in ("qual_short", "qual_long", "seq_empty"):
        return fastq_text(out)
    if kind == "cut":                                     # the quality line is missing
        return fastq_text(recs[:k]) + b"@" + n + b"\n" + s + b"\n+" + p + b"\n" + fastq_text(recs[k + 1:])
    if kind == "multiline":
        return fastq_text(recs[:k]) + b"@" + n + b"\n" + s[:70] + b"\n" + s[70:] + b"\n+" + p + b"\n" + q + b"\n" + fastq_text(recs[k + 1:])
    raise ValueError(kind)


def reported(message, what):
    m = re.search(what + r" (\d+)", message)
    assert m, message
    return int(m.group(1))


def test_fastq_errors(pkg, T):
    rng = random.Random(6)
    recs = fastq_records(rng, 3 * T // 300 + 2)
    second_tile = next(i for i in range(len(recs)) if T < line_start(recs, b"\n", i, 0) and line_start(recs, b"\n", i + 1, 0) < 2 * T)
    for kind in ("no_at", "no_plus", "qual_short", "qual_long", "seq_empty", "cut", "multiline"):
        for k in (0, second_tile, len(recs) - 1):
            text = break_record(recs, k, kind)
            with pytest.raises(R.FastxError) as ei:
                R.fastq(text)
            assert ei.value.record == k
            assert reported(parse_error(pkg, text, "fastq", True), "record") == k
    # two malformed records: the lower one is named, whichever workgroup sees its own first
    for lo, hi in [(1, second_tile), (second_tile, len(recs) - 1), (second_tile + 1, second_tile + 2)]:
        both = list(recs)
        both[lo] = recs[lo][:3] + (recs[lo][3] + b"I",)
        both[hi] = recs[hi][:3] + (recs[hi][3][:-2],)
        assert reported(parse_error(pkg, fastq_text(both), "auto", True), "record") == lo
        text = break_record(both, hi, "no_plus")
        assert reported(parse_error(pkg, text, "auto", True), "record") == lo
    # the last record cut short in every way
    whole = fastq_text(recs)
    assert len(pkg.Records.parse(whole[:-1], "fastq")) == len(recs)      # without its last '\n' the text is still whole
    for cut in (2, 151, 152, 153, 303):
        text = whole[:len(whole) - cut]
        with pytest.raises(R.FastxError) as ei:
            R.fastq(text)
        assert reported(parse_error(pkg, text, "fastq", True), "record") == ei.value.record == len(recs) - 1


def test_fasta_errors_and_slot(pkg, T):
    rng = random.Random(7)
    good = b">a\n" + dna(rng, 100) + b"\n"
    for front in (b"", b"\n\r\n", b"\n" * (T + 5), b"\r\n" * T):
        text = front + b"AC\n" + good
        with pytest.raises(R.FastxError) as ei:
            R.fasta(text)
        assert ei.value.offset == len(front)
        assert reported(parse_error(pkg, text, "fasta", True), "byte") == len(front)
    text = b"\n" * (T - 1) + b"\rAC\n" + good               # a '\r' that is content opens the offending line
    assert reported(parse_error(pkg, text, "fasta", True), "byte") == T - 1
    # the error slot is clear after a good parse
    L = pkg.lib()
    r = pkg.Records.parse(good)
    assert len(r) == 1 and L.sourmash_err_get_last_code() == 0
    h = L.smh_records_parse(good, len(good), 0)
    assert h and L.sourmash_err_get_last_code() == 0
    L.smh_records_free(h)


# ---------------------------------------------------------------------------------------------------------------- 6

@pytest.fixture(scope="module")
def parity_fasta():
    rng = random.Random(8)
    parts = []
    for i in range(200):
        n = rng.choice([0, 5, 20, 26, 30, 31, 40]) if i % 7 == 0 else rng.randrange(0, 5001)
        alphabet = [b"ACGT", b"ACGT", b"acgt", b"ACGTacgt", b"ACGT" * 40 + b"N"][i % 5]
        seq = dna(rng, n, alphabet)
        width = rng.choice([60, 70, 80, 10 ** 6])
        eol = b"\r\n" if i % 11 == 3 else b"\n"
        parts.append(b">contig_%d len=%d" % (i, n) + eol)
        parts.extend(seq[j:j + width] + eol for j in range(0, n, width))
        if i % 13 == 0:
            parts.append(eol)
    text = b"".join(parts)
    return text, R.fasta(text)[0]


MODES = {"scaled31": (0, 31, False, 42, (1 << 64) // 200, False),
         "num21_abund": (500, 21, False, 42, 0, True),
         "protein27": (0, 27, True, 42, (1 << 64) // 50, True)}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_sketch_parity_fasta(pkg, coracle, parity_fasta, mode):
    text, recs = parity_fasta
    parsed = pkg.Records.parse(device_text(text))
    a, b = pkg.KmerMinHash(*MODES[mode]), pkg.KmerMinHash(*MODES[mode])
    a.add_records(parsed, True)
    b.add_sequences(recs, True)
    assert len(a) > 100 and a.mins == b.mins and a.abunds == b.abunds
    if mode == "scaled31":
        o = coracle.MinHash(*MODES[mode])
        for r in recs:
            o.add_sequence(r, True)
        assert a.mins == o.mins
    # force = false: the same reported error k-mer, the same state behind it
    def outcome(fn):
        try:
            fn()
        except pkg.SourmashError as e:
            return e.code, e.message
        return None

    a, b = pkg.KmerMinHash(*MODES[mode]), pkg.KmerMinHash(*MODES[mode])
    got, want = outcome(lambda: a.add_records(parsed, False)), outcome(lambda: b.add_sequences(recs, False))
    assert got == want
    if not MODES[mode][2]:
        assert got is not None and got[0] == 1101 and "N" in got[1]
    assert a.mins == b.mins and a.abunds == b.abunds


def test_sketch_parity_fastq(pkg):
    rng = random.Random(9)
    recs = fastq_records(rng, 400)
    text = fastq_text(recs, b"\r\n")
    parsed = pkg.Records.parse(text)
    assert parsed.format == "fastq"
    a, b = pkg.KmerMinHash(0, 31, False, 42, (1 << 64) // 50, True), pkg.KmerMinHash(0, 31, False, 42, (1 << 64) // 50, True)
    a.add_records(parsed, True)
    b.add_sequences([r[1] for r in recs], True)
    assert len(a) > 100 and a.mins == b.mins and a.abunds == b.abunds


def test_grouped_parity(pkg, parity_fasta):
    text, recs = parity_fasta
    parsed = pkg.Records.parse(text)
    new = lambda: pkg.KmerMinHash(0, 21, False, 42, (1 << 64) // 100, True)   # noqa: E731
    for groups, n in [(None, len(recs)), (np.random.default_rng(10).integers(0, 7, len(recs)), 7)]:
        a, b = [new() for _ in range(n)], [new() for _ in range(n)]
        pkg.KmerMinHash.add_records_grouped(a, parsed, groups, True)
        pkg.KmerMinHash.add_sequences_grouped(b, recs, list(range(n)) if groups is None else groups, True)
        assert sum(len(x) for x in a) > 100
        for x, y in zip(a, b):
            assert x.mins == y.mins and x.abunds == y.abunds
    with pytest.raises(pkg.SourmashError):
        pkg.KmerMinHash.add_records_grouped([new()], parsed, None, True)       # one sketch per record, or groups


# ---------------------------------------------------------------------------------------------------------------- 7

def test_read_text_gzip(pkg, parity_fasta, tmp_path):
    text, recs = parity_fasta
    plain, packed = tmp_path / "a.fa", tmp_path / "a.fa.gz"
    plain.write_bytes(text)
    with gzip.open(packed, "wb") as fh:
        fh.write(text)
    assert pkg.fastx.read_text(str(plain)) == text and pkg.fastx.read_text(str(packed)) == text
    a, b = pkg.Records.parse(pkg.fastx.read_text(str(plain))), pkg.Records.parse(pkg.fastx.read_text(str(packed)))
    assert len(a) == len(b) == len(recs) and np.array_equal(a.offsets, b.offsets)
    assert torch.equal(a.seq_tensor(), b.seq_tensor())
    assert b.names(text)[3] == b"contig_3 len=%d" % len(recs[3])


# ---------------------------------------------------------------------------------------------------------------- 8

def test_past_4_gib(pkg):
    """A 63 MiB block of wrapped FASTA (64 records of 1 024 000 bases, 80 columns), repeated on the device to 4.57 GiB:
    positions past 2^32 in the text, in the compacted bytes and in the offsets."""
    n_b, lines_per, width = 64, 12800, 80
    rng = np.random.default_rng(11)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n_b, lines_per, width), dtype=np.uint8)]
    body = np.concatenate([bases, np.full((n_b, lines_per, 1), 0x0A, dtype=np.uint8)], axis=2).reshape(n_b, -1)
    heads = np.frombuffer(b"".join(b">r%05d\n" % i for i in range(n_b)), dtype=np.uint8).reshape(n_b, 8)
    block = np.ascontiguousarray(np.concatenate([heads, body], axis=1)).reshape(-1)
    per = lines_per * width
    total_b = n_b * per
    offsets_b = np.arange(n_b + 1, dtype=np.uint64) * np.uint64(per)
    repeats = (9 << 29) // block.size + 2
    assert repeats * block.size > (9 << 29) and repeats * total_b > (1 << 32)

    text = torch.from_numpy(block).cuda().repeat(repeats)
    parsed = pkg.Records.parse(text, "fasta")
    del text
    assert len(parsed) == repeats * n_b and parsed.total == repeats * total_b
    want = (np.arange(repeats, dtype=np.uint64)[:, None] * np.uint64(total_b) + offsets_b[None, :n_b]).reshape(-1)
    off = parsed.offsets
    assert np.array_equal(off[:-1], want) and int(off[-1]) == repeats * total_b
    start, length = parsed.name_spans()
    assert int(start[-1]) == (repeats - 1) * block.size + (n_b - 1) * (8 + lines_per * (width + 1)) + 1
    assert np.all(length == 6)

    mx = (1 << 64) // 1000
    whole, one = pkg.KmerMinHash(0, 31, False, 42, mx, True), pkg.KmerMinHash(0, 31, False, 42, mx, True)
    whole.add_records(parsed, True)
    flat = torch.from_numpy(np.ascontiguousarray(bases).reshape(-1)).cuda()   # the block's bases, cut by construction
    one.add_sequences_dev(flat.data_ptr(), total_b, offsets_b, True)
    assert len(one) > 10000 and np.array_equal(whole.mins_np(), one.mins_np())
    assert np.array_equal(whole.abunds_np(), one.abunds_np() * np.uint64(repeats))
