"""The format rules of the device parser (include/sourmash_amd.h, "Records cut out of FASTA / FASTQ text"), restated in
plain Python: the yardstick of tests/test_gpu_fastx.py, itself pinned on literals by tests/test_fastx_rules.py.

  lines(text)  -> [(start, end)]: every line's content is text[start:end], terminator removed
  fasta(text)  -> (records, spans)      raises FastxError with .offset (byte offset of the data in front of the first header)
  fastq(text)  -> (records, spans)      raises FastxError with .record (lowest malformed record, 0-based)
  parse(text, fmt) with fmt in auto / fasta / fastq -> (format, records, spans)

records are bytes objects; spans are the names as (start, length) into the text."""


class FastxError(Exception):
    def __init__(self, message, offset=None, record=None):
        super().__init__(message)
        self.offset = offset
        self.record = record


def lines(text):
    """A line ends at '\\n'; one '\\r' directly in front of it, or a '\\r' that is the text's last byte, belongs to the
    terminator; a last line without '\\n' exists if it holds at least one byte."""
    out = []
    p, n = 0, len(text)
    while p < n:
        q = text.find(b"\n", p)
        if q < 0:
            end = n - 1 if text[n - 1] == 0x0D else n
            out.append((p, end))
            break
        end = q - 1 if q > p and text[q - 1] == 0x0D else q
        out.append((p, end))
        p = q + 1
    return out


def fasta(text):
    records, spans = [], []
    cur = None
    for s, e in lines(text):
        if e == s:
            continue                                   # empty lines are ignored everywhere
        if text[s] == 0x3E:                            # '>' as the FIRST byte of a line
            if cur is not None:
                records.append(b"".join(cur))
            cur = []
            spans.append((s + 1, e - s - 1))
        else:
            if cur is None:
                raise FastxError("data in front of the first header at byte %d" % s, offset=s)
            cur.append(text[s:e])
    if cur is not None:
        records.append(b"".join(cur))
    return records, spans


def fastq(text):
    ls = lines(text)
    while ls and ls[-1][0] == ls[-1][1]:
        ls.pop()                                       # empty lines at the end are dropped
    if len(ls) % 4 == 3 and ls[-2][0] == ls[-2][1]:
        ls.append((len(text), len(text)))              # the empty quality line of a last, empty record
    records, spans = [], []
    for r in range((len(ls) + 3) // 4):
        rec = ls[4 * r:4 * r + 4]
        bad = len(rec) < 4
        if not bad:
            (hs, he), (ss, se), (ps, pe), (qs, qe) = rec
            bad = he == hs or text[hs] != 0x40 or pe == ps or text[ps] != 0x2B or qe - qs != se - ss
        if bad:
            raise FastxError("malformed record %d" % r, record=r)
        records.append(text[ss:se])
        spans.append((hs + 1, he - hs - 1))
    return records, spans


def sniff(text):
    """The first byte of the first non-empty line: '>' FASTA, '@' FASTQ.  A text without one holds no records."""
    for s, e in lines(text):
        if e > s:
            if text[s] == 0x3E:
                return "fasta"
            if text[s] == 0x40:
                return "fastq"
            raise FastxError("neither FASTA nor FASTQ")
    return "fasta"


def parse(text, fmt="auto"):
    text = bytes(text)
    if fmt == "auto":
        fmt = sniff(text)
    records, spans = (fasta if fmt == "fasta" else fastq)(text)
    return fmt, records, spans
