"""The compile-time-k two-limb DNA kernels (k = 31, 21) choose the hashed strand with one floating-point minimum of the
two windows' bit patterns.  Every hash against the C oracle (max_hash = 2^64 - 1, nothing filtered out) on the inputs
where that could go wrong: windows with 1, 2, ... k leading zero digits (small ones are denormal doubles, the all-A window
is +0.0) on the forward strand (runs of A at the k-mer's right end), on the reverse complement (runs of T at its left
end) and on both; poly-A and poly-T; and pairs of windows that are as close as two strands can be.  The forward window
and the reverse complement's differ in digit i exactly when they differ in digit k - 1 - i, and for an odd k always in
the middle digit: the closest pairs differ in the middle digit alone (the lowest digit that can differ alone), and in
the highest, the lowest and the middle one.  Records shorter than a lane's run, records that end inside one and one long
record; upper and lower case; one N in each record with force = true.  The coverage is asserted on the CPU."""
import random

import pytest

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rc(s):
    return s.translate(COMP)[::-1]


def rnd(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def records(ksize):
    rng = random.Random(1000 + ksize)
    recs = []
    for j in range(1, ksize + 1):
        # a run of j A's closed by C on both sides: windows with 1..j leading zero digits, forward; T's: the other strand
        recs.append(rnd(rng, ksize + 3) + b"C" + b"A" * j + b"C" + rnd(rng, ksize + 3))
        recs.append(rnd(rng, ksize + 3) + b"G" + b"T" * j + b"G" + rnd(rng, ksize + 3))
        if 2 * j < ksize:
            mid = rnd(rng, ksize - 2 * j - 2) if ksize - 2 * j >= 2 else b""
            core = (b"G" + mid + b"C")[:ksize - 2 * j]
            recs.append(b"T" * j + core + b"A" * j)                       # exactly one k-mer: a record as short as can be
            recs.append(rnd(rng, 5) + b"C" + b"T" * j + core + b"A" * j + b"G" + rnd(rng, 5))
    recs += [b"A" * ksize, b"T" * ksize, b"A" * 200, b"T" * 333, b"A" * 150 + b"T" * 150, b"T" * 150 + b"A" * 150]
    # near-palindromes: h + m + rc(h) differs from its reverse complement in the middle digit alone; with the outer pair
    # (first, last letter) not complementary, in the highest and the lowest digit too
    half = (ksize - 1) // 2
    for _ in range(6):
        h = rnd(rng, half)
        for m in b"ACGT":
            recs.append(h + bytes([m]) + rc(h))
            for first in b"ACGT":
                for last in b"ACGT":
                    recs.append(bytes([first]) + h[1:] + bytes([m]) + rc(h)[:-1] + bytes([last]))
    # the same through longer records: every record so far, joined in chunks (records that end inside a run of 128)
    # and all in one (long runs of clean groups)
    short = list(recs)
    for a in range(0, len(short), 7):
        recs.append(b"".join(short[a:a + 7]))
    recs.append(b"".join(short))
    assert all(len(r) >= ksize for r in recs)
    return recs


def variants(recs, ksize):
    """upper case, lower case, and one N in every record (force = true skips the windows that hold it)"""
    rng = random.Random(77 + ksize)
    out = []
    for r in recs:
        out.append(r)
        out.append(r.lower())
        at = rng.randrange(len(r))
        out.append(r[:at] + b"N" + r[at + 1:])
        out.append((r[:at] + b"n" + r[at + 1:]).lower() if at % 2 else r[:at].lower() + b"N" + r[at + 1:])
    return out


def leading_zero_coverage(recs, ksize):
    """leading zero digits of the forward window (A's at the right end) and of the reverse complement's (T's at the left
    end) over the valid windows; and the windows' closest pairs"""
    fwd, rev, both, close = set(), set(), set(), set()
    for r in recs:
        u = r.upper()
        for i in range(len(u) - ksize + 1):
            km = u[i:i + ksize]
            if km.strip(b"ACGT"):
                continue
            a = ksize - len(km.rstrip(b"A"))
            t = ksize - len(km.lstrip(b"T"))
            fwd.add(a)
            rev.add(t)
            if a and t:
                both.add((t, a))
            diff = [q for q in range(ksize) if km[q] != rc(km)[q]]
            if len(diff) <= 3:
                close.add(tuple(diff))
    return fwd, rev, both, close


@pytest.mark.parametrize("ksize", (31, 21))
def test_strand_choice_on_small_and_close_windows(pkg, coracle, ksize):
    recs = variants(records(ksize), ksize)
    fwd, rev, both, close = leading_zero_coverage(recs, ksize)
    assert fwd == set(range(ksize + 1)) and rev == set(range(ksize + 1))
    assert {(j, j) for j in range(1, (ksize + 1) // 2)} <= both
    mid = (ksize - 1) // 2
    assert (mid,) in close and (0, mid, ksize - 1) in close
    case = (0, ksize, False, 42, (1 << 64) - 1, True)
    g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
    g.add_sequences(recs, True)
    for r in recs:
        o.add_sequence(r, True)
    assert len(o.mins) > 5000
    assert g.mins == o.mins
    assert g.abunds == o.abunds


@pytest.mark.parametrize("ksize", (31, 21))
def test_strand_choice_grouped_bottom_num(pkg, coracle, ksize):
    """the per-record kernel: a grouped bottom-num batch whose sketches are large enough to keep every hash"""
    recs = variants(records(ksize), ksize)
    groups = [i % 3 for i in range(len(recs))]
    case = (200000, ksize, False, 42, 0, True)
    gs = [pkg.KmerMinHash(*case) for _ in range(3)]
    os_ = [coracle.MinHash(*case) for _ in range(3)]
    pkg.KmerMinHash.add_sequences_grouped(gs, recs, groups, True)
    for r, grp in zip(recs, groups):
        os_[grp].add_sequence(r, True)
    for g, o in zip(gs, os_):
        assert len(o.mins) > 2000
        assert g.mins == o.mins
        assert g.abunds == o.abunds
