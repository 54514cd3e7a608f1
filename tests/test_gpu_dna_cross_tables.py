"""The k2 words of the two-limb DNA kernels take the high dword's cross term from the tables ({T2'', a.hi} for the low
half, {B, B'} for the high half).  Every hash against the C oracle (max_hash = 2^64 - 1, nothing filtered out) on inputs
built by enumeration: for each k2 word position of the k-mer (word 1 = letters 8..15, word 3 = letters 24..), every value
of the low half x every value of the high half, embedded in an otherwise fixed k-mer whose strand is pinned (eight
leading A's: the k-mer is smaller than its reverse complement, so it is the one hashed).  Each k-mer is a record of its
own, fed together with its reverse complement, which brings the same canonical k-mer through the other strand.
The coverage is asserted on the CPU from the canonical k-mers: all 256 x 4^nb pairs, and for every high-half value both
a wrap of a.hi + B and none (where the arithmetic allows one: see check_coverage).
k = 31, 21 (compile-time), 19, 25, 27, 29, 30, 32 (run-time): the partial group in a low half (19: k1 word, 25, 27: k2
word) and in a high half (21: k1 word, 29, 30, 31: k2 word).  One grouped bottom-num batch runs the per-record kernel."""
import pytest

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGT", b"TGCA")
C2 = 0x4CF5AD432745937F
M32 = (1 << 32) - 1
# words 0..3 of the fixed k-mer.  Word 0 is all A: with at most eight T's at the end (and then letter 8 = A below the
# complement of letter 23 = C) the reverse complement is the larger strand.  Every k of the test ends on a letter that is
# not T when the end is not enumerated.
FIXED = [b"AAAAAAAA", b"ACGTCAGC", b"GCAGACGC", b"CAGGCGAC"]
KSIZES = (19, 21, 25, 27, 29, 30, 31, 32)
CASES = [(k, w) for k in KSIZES for w in (1, 3) if 8 * w < k]


def quad(idx, nb):
    return bytes(b"ACGT"[(idx >> (2 * j)) & 3] for j in range(nb))


def kmers_for(ksize, word):
    """(k-mers, letters of the low half, letters of the high half): every low half x every high half of the word"""
    n_lo = min(4, ksize - 8 * word)
    n_hi = max(0, min(4, ksize - 8 * word - 4))
    lows = [quad(i, n_lo) for i in range(4 ** n_lo)]
    highs = [quad(i, n_hi) for i in range(4 ** n_hi)]
    head = b"".join(FIXED[:word])
    tail = b"".join(FIXED[word + 1:])
    return [(head + lo + hi + tail)[:ksize] for lo in lows for hi in highs], n_lo, n_hi


def ascii_word(q):
    return int.from_bytes(q, "little")


def check_coverage(kmers, ksize, word, n_lo, n_hi):
    pairs, wrap, nowrap = set(), set(), set()
    for km in kmers:
        assert len(km) == ksize
        rc = km.translate(COMP)[::-1]
        assert km < rc                                    # the strand is pinned: the k-mer itself is hashed
        lo, hi = km[8 * word:8 * word + n_lo], km[8 * word + 4:8 * word + 4 + n_hi]
        pairs.add((lo, hi))
        if n_hi:
            a_hi = (ascii_word(lo) * C2 >> 32) & M32
            b = (ascii_word(hi) * C2) & M32
            (wrap if a_hi + b > M32 else nowrap).add(hi)
    assert len(pairs) == len(kmers) == 4 ** n_lo * 4 ** n_hi
    if n_hi:
        # every high-half value without a wrap of a.hi + B and with one -- but for "TAA" and "TCG" as the k-mer's last
        # three letters: their B (0x86a4ac, 0xa7a2ac) is below 2^32 - the largest a.hi of any low half (0xff379448)
        assert len(nowrap) == 4 ** n_hi
        assert set(quad(i, n_hi) for i in range(4 ** n_hi)) - wrap == ({b"TAA", b"TCG"} if n_hi == 3 else set())


def both_strands(kmers):
    recs = []
    for km in kmers:
        recs.append(km)
        recs.append(km.translate(COMP)[::-1])
    return recs


@pytest.mark.parametrize("ksize,word", CASES)
def test_every_half_pair_of_a_k2_word(pkg, coracle, ksize, word):
    kmers, n_lo, n_hi = kmers_for(ksize, word)
    check_coverage(kmers, ksize, word, n_lo, n_hi)
    recs = both_strands(kmers)
    case = (0, ksize, False, 42, (1 << 64) - 1, True)
    g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
    g.add_sequences(recs, True)
    for r in recs:
        o.add_sequence(r, True)
    assert len(o.mins) == len(kmers)                      # (no two of them collide)
    assert g.mins == o.mins
    assert g.abunds == o.abunds == [2] * len(kmers)


@pytest.mark.parametrize("ksize", (31, 21))
def test_grouped_bottom_num_batch(pkg, coracle, ksize):
    """smh_add_sequences_grouped on bottom-num sketches large enough to keep every hash: the per-record kernel"""
    kmers, n_lo, n_hi = kmers_for(ksize, 3 if ksize > 24 else 1)
    kmers = kmers[:16384]
    recs = both_strands(kmers)
    groups = [(i // 2) % 4 for i in range(len(recs))]
    case = (40000, ksize, False, 42, 0, True)
    gs = [pkg.KmerMinHash(*case) for _ in range(4)]
    os_ = [coracle.MinHash(*case) for _ in range(4)]
    pkg.KmerMinHash.add_sequences_grouped(gs, recs, groups, True)
    for r, grp in zip(recs, groups):
        os_[grp].add_sequence(r, True)
    for g, o in zip(gs, os_):
        assert len(o.mins) == len(kmers) // 4
        assert g.mins == o.mins
        assert g.abunds == o.abunds
