"""The FASTA / FASTQ format rules, pinned on literals: tests/fastx_restatement.py is the yardstick of the device parser's
tests, so it is checked itself here.  No GPU needed; the last test is the no-GPU behaviour of the C ABI."""
import ctypes as C

import pytest

import fastx_restatement as R


def names(text, spans):
    return [text[s:s + n] for s, n in spans]


def test_lines():
    assert R.lines(b"") == []
    assert R.lines(b"\n") == [(0, 0)]
    assert R.lines(b"ab") == [(0, 2)]
    assert R.lines(b"ab\r") == [(0, 2)]                 # a '\r' that is the last byte belongs to the terminator
    assert R.lines(b"a\rb\r\r\nc\n") == [(0, 4), (6, 7)]  # only ONE '\r' in front of '\n' does
    assert R.lines(b"\r\n\r") == [(0, 0), (2, 2)]
    assert R.lines(b" \t\n") == [(0, 2)]


def test_fasta_literals():
    text = b"\n\r\n>a\r\nAC\r\nGT\n\n>b\n>c d\nA>C\rG\r"
    recs, spans = R.fasta(text)
    assert recs == [b"ACGT", b"", b"A>C\rG"]
    assert names(text, spans) == [b"a", b"b", b"c d"]
    recs, spans = R.fasta(b">a")
    assert recs == [b""] and spans == [(1, 1)]
    assert R.fasta(b"") == ([], [])
    assert R.fasta(b"\n\r\n\n") == ([], [])
    with pytest.raises(R.FastxError) as ei:
        R.fasta(b"AC\n>a\n")
    assert ei.value.offset == 0
    with pytest.raises(R.FastxError) as ei:
        R.fasta(b"\n\r\n AC\n>a\n")
    assert ei.value.offset == 3


def test_fastq_literals():
    text = b"@r1\nACGT\n+\n@@@@\n@r2 x\r\nAC\r\n+r2 x\r\n+>\r\n\n\n"
    recs, spans = R.fastq(text)
    assert recs == [b"ACGT", b"AC"]
    assert names(text, spans) == [b"r1", b"r2 x"]
    for text in (b"@e\n\n+\n\n", b"@e\n\n+"):
        recs, spans = R.fastq(text)
        assert recs == [b""] and names(text, spans) == [b"e"]
    assert R.fastq(b"") == ([], [])
    assert R.fastq(b"\n\n") == ([], [])


@pytest.mark.parametrize("text,record", [
    (b"@a\nACGT\n+\nIII\n", 0),                          # quality one byte short
    (b"a\nACGT\n+\nIIII\n", 0),                          # no '@'
    (b"@a\nACGT\n-\nIIII\n", 0),                         # '-' in place of '+'
    (b"@a\nACGT\n+\nIIII\n@b\nAC\n+\n", 1),              # second record cut after '+'
])
def test_fastq_malformed(text, record):
    with pytest.raises(R.FastxError) as ei:
        R.fastq(text)
    assert ei.value.record == record


def test_fastq_more_malformed():
    for text, record in [(b"@a\nAC\nGT\n+\nIIII\n", 0),             # multi-line FASTQ
                         (b"@a\nAC\n+\nII\n@b\n", 1),               # fewer lines than a record needs
                         (b"@a\nAC\n+\nII\n\n@b\nAC\n+\nII\n", 1),  # an empty line between records shifts the roles
                         (b"@a\nAC\n+\n", 0)]:                      # three lines, but the sequence is not empty
        with pytest.raises(R.FastxError) as ei:
            R.fastq(text)
        assert ei.value.record == record


def test_sniff():
    assert R.parse(b"\n\r\n>a\nAC\n")[0] == "fasta"
    assert R.parse(b"@a\nAC\n+\nII\n")[0] == "fastq"
    assert R.sniff(b"\n@a\nAC\n+\nII\n") == "fastq"     # ... where the empty first line then makes record 0 malformed
    with pytest.raises(R.FastxError) as ei:
        R.parse(b"\n@a\nAC\n+\nII\n")
    assert ei.value.record == 0
    assert R.parse(b"") == ("fasta", [], [])
    with pytest.raises(R.FastxError):
        R.parse(b"AC\n")


def test_parse_fails_loudly_without_gpu(pkg):
    if pkg.device_available():
        pytest.skip("a GPU is present")
    L = pkg.lib()
    L.sourmash_err_clear()
    text = b">a\nACGT\n"
    assert L.smh_records_parse(text, len(text), 0) is None
    assert L.sourmash_err_get_last_code() == 2
    with pytest.raises(pkg.SourmashError) as ei:
        pkg.Records.parse(text)
    assert ei.value.code == 2 and "no HIP device" in ei.value.message
    L.sourmash_err_clear()
    assert L.smh_records_parse_dev(C.c_void_p(0), 0, 1, C.c_void_p(0)) is None
    assert L.sourmash_err_get_last_code() == 2
    L.sourmash_err_clear()
    assert L.smh_records_tile_bytes() > 0
    assert L.smh_records_len(None) == 0 and L.smh_records_total(None) == 0
