"""Every hash of the rolling DNA kernel against the C oracle (max_hash = 2^64 - 1, nothing filtered out), on an order-8
de Bruijn sequence over ACGT and its reverse complement.  At least 245 of the 256 4-letter values reach every full
half-word position of the hashed (canonical) k-mers, and 56-65 % of the 65 536 8-letter values every full word position;
the test asserts both counts.  This checks the folded table entries of the two-limb kernels (k = 31, 21 and the run-time
k <= 32, with the k-mer's partial group of letters in a low half at k = 19 and 27 and in a high half at k = 21, 29 and
31) and the plain tables of the four-limb ones (k = 40, 51)."""
import pytest

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def de_bruijn_acgt(n):
    """The lexicographically least de Bruijn sequence B(4, n), made linear: every n-letter string over ACGT occurs once."""
    a = [0] * (4 * n)
    seq = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    s = bytes(b"ACGT"[d] for d in seq)
    return s + s[:n - 1]


def word_coverage(recs, ksize):
    """{word position: distinct 8-letter values} over the full words of the canonical k-mers that are hashed, and the
    fewest distinct 4-letter values over the full half-word positions"""
    cov = {w: set() for w in range(ksize // 8)}
    halves = {h: set() for h in range(ksize // 4)}
    for r in recs:
        rc = r.translate(COMP)[::-1]
        n = len(r)
        for i in range(n - ksize + 1):
            f = r[i:i + ksize]
            b = rc[n - i - ksize:n - i]
            c = f if f < b else b
            for w in cov:
                cov[w].add(c[8 * w:8 * w + 8])
            for h in halves:
                halves[h].add(c[4 * h:4 * h + 4])
    return {w: len(v) for w, v in cov.items()}, min(len(v) for v in halves.values())


SEQ = de_bruijn_acgt(8)
RECS = [SEQ, SEQ.translate(COMP)[::-1]]

# word_coverage() on RECS: distinct values per full word position (of 4^8 = 65536), fewest per full half (of 256)
COVERAGE = {
    19: ({0: 37138, 1: 39835}, 245),
    21: ({0: 37536, 1: 39742}, 249),
    27: ({0: 37104, 1: 40823, 2: 40883}, 245),
    29: ({0: 36951, 1: 40724, 2: 40714}, 251),
    31: ({0: 36923, 1: 40320, 2: 40413}, 256),
    40: ({0: 38804, 1: 39231, 2: 40816, 3: 39242, 4: 38825}, 254),
    51: ({0: 38319, 1: 41872, 2: 42455, 3: 41101, 4: 42527, 5: 41896}, 247),
}


@pytest.mark.parametrize("ksize", sorted(COVERAGE))
def test_every_hash_on_de_bruijn_input(pkg, coracle, ksize):
    assert len(SEQ) == 65536 + 7
    assert word_coverage(RECS, ksize) == COVERAGE[ksize]
    case = (0, ksize, False, 42, (1 << 64) - 1, True)
    g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
    g.add_sequences(RECS, True)
    for r in RECS:
        o.add_sequence(r, True)
    assert len(o.mins) > 60000
    assert g.mins == o.mins
    assert g.abunds == o.abunds
