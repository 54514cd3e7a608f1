"""The sketch kernels' filter on the sum of the two open mixes (murmur_device.hpp: open_hi_sum1<true> against
open_thr<true>; k_dna_rolling and k_protein_fused), on the GPU, with thresholds that sit ON hashes of the input.

The filter's value E is the digest's high dword plus 0, 1 or 2 (tests/test_open_sum_identity.py).  A window of class
c = E - h.hi is the one that a threshold rule of thr.hi + c' with c' < c would lose at max_hash = h, so every kernel
family is run with max_hash = h and max_hash = h - 1 for at least four windows h of EACH class, and with the edge values
of open_thr.  The class of every window is worked out on the CPU from its hashed string (tests/open_sum_restatement.py,
whose murmur is asserted equal to the oracle's on every string), and every class is asserted present with four members
before the GPU is asked anything.  A sketch must equal the full sketch (max_hash = 2^64 - 1: every hash, with its
abundance) cut at the threshold; at max_hash = 0, which the reference does not read as a threshold, the oracle's own
run.

One seeded record of 3 000 bases (or residues): one tile per call.  Families: DNA at k = 31, 21 (compile-time), 29, 32
(run-time, two limbs), 51, 40 (four limbs), 70 (eight limbs); a grouped bottom-num batch, which runs the per-record
kernels (k = 29, 51, 70 took the new filter; k = 31 keeps the one on both products and is run all the same);
translated protein at ksize 27, 21, 30; amino-acid input at windows 7, 9, 10, 16 and 12 over the three alphabets.
k_amino_tiled keeps the filter on both products (the one on the sum was measured there and was no gain), and its
run-time window, 12, closes the digest and filters nothing: these cases pin the thresholds of the kernels that did not
change.  The protein and amino-acid windows are classified like the DNA ones.

Grouped batch: a group's threshold is its full sketch's largest hash, so a group is a bottom-num sketch filled beforehand
with every hash of the record up to h and, on top, h + 1 (num = their count): the kernel's threshold for the group's
record is h + 1, in h's own high dword, and the window that hashes to h shows in its abundance, 1 + its count in the
record.  A second group per h stops at h itself: the threshold is h, which a full bottom-num sketch never counts again.
No edge values there: the thresholds are what a sketch can hold."""
import random

import numpy as np
import pytest

import amino_restatement as ar
import open_sum_restatement as osr

pytestmark = pytest.mark.gpu

MAXH = (1 << 64) - 1
EDGES = (0, (1 << 32) - 1, 0xFFFFFFFC_FFFFFFFF, 0xFFFFFFFD_00000000, 0xFFFFFFFE_FFFFFFFF, MAXH)
PER_CLASS = 4
N = 3000
RNG = random.Random(31)
DNA = bytes(RNG.choice(b"ACGT") for _ in range(N))
RESIDUES = bytes(RNG.choice(ar.LETTERS.encode()) for _ in range(N))


def dna_words(ksize):
    return [min(DNA[i:i + ksize], osr.pyoracle.revcomp(DNA[i:i + ksize])) for i in range(N - ksize + 1)]


def translated_words(ksize):
    w, out = ksize // 3, []
    rc = osr.pyoracle.revcomp(DNA)
    for frame in range(3):
        for strand in (DNA, rc):
            aa = osr.pyoracle.to_aa(strand[frame:])
            out += [aa[i:i + w] for i in range(len(aa) - w + 1)]
    return out


def amino_words(alpha, w):
    e = ar.encode(RESIDUES, alpha)
    return [e[i:i + w] for i in range(len(e) - w + 1)]


def thresholds_by_class(words):
    """{class: PER_CLASS hashes of that class, spread over the sorted hashes}; asserts that every class has that many"""
    by_class = {0: set(), 1: set(), 2: set()}
    for word in set(words):
        h, c = osr.classify(word)
        by_class[c].add(h)                                 # (KeyError: a class outside 0, 1, 2)
    picked = {}
    for c, hs in by_class.items():
        hs = sorted(hs)
        assert len(hs) >= PER_CLASS, (c, len(hs))
        picked[c] = [hs[(len(hs) - 1) * j // (PER_CLASS - 1)] for j in range(PER_CLASS)]
    return picked


def full_state(words):
    mins, abunds = ar.full_state([osr.pyoracle.hash_murmur(w, 42) for w in words])
    return mins, abunds


def check_scaled_family(words, full_mins, full_abunds, sketch_at, oracle_at):
    """sketch_at(max_hash) -> library sketch of the record; oracle_at(max_hash) -> oracle sketch of the record"""
    mins, abunds = full_state(words)
    assert (mins == full_mins).all() and (abunds == full_abunds).all()      # the oracle's full sketch gives every hash
    picked = thresholds_by_class(words)
    for c, hs in picked.items():
        for h in hs:
            for mx in (h, h - 1):
                g = sketch_at(mx)
                keep = mins <= np.uint64(mx)
                assert keep.sum() >= 1 or mx < int(mins[0])
                gm, ga = g.mins_np(), g.abunds_np()
                assert gm.shape == mins[keep].shape and (gm == mins[keep]).all(), (c, hex(h), hex(mx))
                assert (ga == abunds[keep]).all(), (c, hex(h), hex(mx))
                assert (h in set(gm.tolist())) == (mx == h)
    for mx in EDGES:
        g, o = sketch_at(mx), oracle_at(mx)
        ar.same_state(g, o)
        if mx:
            keep = mins <= np.uint64(mx)
            assert (g.mins_np() == mins[keep]).all()


# ------------------------------------------------------------------------------------------------------------------
# DNA

@pytest.mark.parametrize("ksize", [31, 21, 29, 32, 51, 40, 70])
def test_dna(pkg, coracle, ksize):
    def sketch_at(mx):
        g = pkg.KmerMinHash(0, ksize, False, 42, mx, True)
        g.add_sequence(DNA, True)
        return g

    def oracle_at(mx):
        o = coracle.MinHash(0, ksize, False, 42, mx, True)
        o.add_sequence(DNA, True)
        return o

    full = oracle_at(MAXH)
    check_scaled_family(dna_words(ksize), full.mins_np(), full.abunds_np(), sketch_at, oracle_at)


@pytest.mark.parametrize("ksize", [29, 51, 70, 31])
def test_dna_grouped_bottom_num(pkg, coracle, ksize):
    words = dna_words(ksize)
    mins, abunds = full_state(words)
    picked = thresholds_by_class(words)
    hs = [(h, top) for c in (0, 1, 2) for h in picked[c] for top in (h + 1, h)]
    gs, os_ = [], []
    for h, top in hs:
        fill = [int(x) for x in mins[mins <= np.uint64(h)]]
        assert fill[-1] == h and (top >> 32) == (h >> 32)
        if top != h:
            fill.append(top)
        g, o = pkg.KmerMinHash(len(fill), ksize, False, 42, 0, True), coracle.MinHash(len(fill), ksize, False, 42, 0, True)
        g.add_many(fill); o.add_many(fill)
        gs.append(g); os_.append(o)
    pkg.KmerMinHash.add_sequences_grouped(gs, [DNA] * len(hs), list(range(len(hs))), True)
    for (h, top), g, o in zip(hs, gs, os_):
        o.add_sequence(DNA, True)
        ar.same_state(g, o)
        # every window up to h counted once more; the sketch's largest hash never is (the reference's add_hash takes a hash
        # into a full bottom-num sketch only when it is BELOW the largest): h itself when it is the largest
        keep = mins <= np.uint64(h)
        want = abunds[keep] + np.uint64(1)
        if top == h:
            want[-1] = 1
        else:
            want = np.append(want, np.uint64(1))
        assert (g.abunds_np() == want).all() and int(g.mins_np()[-1]) == top, (hex(h), hex(top))


# ------------------------------------------------------------------------------------------------------------------
# translated protein (k_protein_fused) and amino-acid input (k_amino_tiled)

@pytest.mark.parametrize("ksize", [27, 21, 30])
def test_translated_protein(pkg, coracle, ksize):
    def sketch_at(mx):
        g = pkg.KmerMinHash(0, ksize, True, 42, mx, True)
        g.add_sequence(DNA, True)
        return g

    def oracle_at(mx):
        o = coracle.MinHash(0, ksize, True, 42, mx, True)
        o.add_sequence(DNA, True)
        return o

    c = ar.counters(pkg, lambda: sketch_at(MAXH).mins_np())   # (a single record is queued until the sketch is read)
    assert c["protein_fused"] >= 1 and c["translate"] == 0 and c["hash_windows"] == 0, c
    full = oracle_at(MAXH)
    check_scaled_family(translated_words(ksize), full.mins_np(), full.abunds_np(), sketch_at, oracle_at)


@pytest.mark.parametrize("alpha", ar.ALPHABETS)
@pytest.mark.parametrize("w", [7, 9, 10, 16, 12])
def test_amino_acid_input(pkg, alpha, w):
    def sketch_at(mx):
        g = pkg.KmerMinHash(0, 3 * w, True, 42, mx, True, alphabet=alpha)
        g.add_protein(RESIDUES)
        return g

    words = amino_words(alpha, w)
    hashes = [osr.pyoracle.hash_murmur(word, 42) for word in words]

    def oracle_at(mx):                                     # ar.amino_sketch with the windows hashed once
        o = ar.new_sketch(3 * w, 0, mx)
        o.add_many(hashes)
        return o

    c = ar.counters(pkg, lambda: sketch_at(MAXH).mins_np())
    assert c["amino_tiled"] == 1 and c["amino_generic"] == 0, c
    full = oracle_at(MAXH)
    check_scaled_family(words, np.asarray(full.mins, dtype=np.uint64), np.asarray(full.abunds, dtype=np.uint64),
                        sketch_at, oracle_at)
