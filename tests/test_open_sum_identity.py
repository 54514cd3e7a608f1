"""The sketch kernels' filter on the sum of the two open mixes, in Python integers (tests/open_sum_restatement.py states it
the way the kernel forms it: the 64-bit sum, two multiply-adds whose low dwords are used, one multiply-high, one 32-bit
add).  With d = (ka + kb) * C:  E == d.hi + 1;  E - h.hi is 0, 1 or 2 (= 1 + cy - cy');  h <= thr implies
E <= open_thr(thr), which saturates to all ones for thr.hi >= 0xfffffffd.  Pairs are built backwards from chosen
products and chosen digests through C^-1 mod 2^64, so that every combination of the two carries and of a wrap of
a.hi + b.hi is there, and digests sit on both sides of every threshold.  No GPU needed."""
import random

import open_sum_restatement as osr
from open_sum_restatement import M32, M64

FIXED = (0, 1, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1)
THRESHOLDS = [(hi << 32) | lo for hi in (0, 1, 1 << 22, 0xFFFFFFFC, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF) for lo in (0, M32)]
EDGE32 = (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF)


def build_pairs():
    rng = random.Random(20)
    pairs = [(ka, kb) for ka in FIXED for kb in FIXED]
    pairs += [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(20000)]
    # chosen products: every edge value in every dword of a and of b
    for ah in EDGE32:
        for bh in EDGE32:
            for al in EDGE32:
                for bl in EDGE32:
                    pairs.append(osr.pair_from_products((ah << 32) | al, (bh << 32) | bl))
    # chosen digests: at and around every threshold, split at random and at the edges
    for thr in THRESHOLDS:
        for delta in (-2, -1, 0, 1, 2, -(1 << 32), 1 << 32, -(1 << 33), 1 << 33):
            h = (thr + delta) & M64
            for a_shifted in (0, 1, M32, 1 << 32, M64, h, (h + 1) & M64):
                pairs.append(osr.pair_with_digest(h, a_shifted))
            for _ in range(40):
                pairs.append(osr.pair_with_digest(h, rng.getrandbits(64)))
        for _ in range(400):                              # anywhere below the threshold
            pairs.append(osr.pair_with_digest(rng.randint(0, thr), rng.getrandbits(64)))
    return pairs


PAIRS = build_pairs()


def test_pairs_built_backwards_are_what_they_claim():
    rng = random.Random(21)
    assert (osr.C * osr.C_INV) & M64 == 1
    for _ in range(2000):
        a, b, h = rng.getrandbits(64), rng.getrandbits(64), rng.getrandbits(64)
        assert osr.products(*osr.pair_from_products(a, b)) == (a, b)
        ka, kb = osr.pair_with_digest(h, a)
        assert osr.open_full(ka, kb) == h
        pa, _ = osr.products(ka, kb)
        assert pa ^ (pa >> 33) == a


def test_e_is_the_high_dword_of_one_product_plus_one():
    for ka, kb in PAIRS:
        d = ((ka + kb) * osr.C) & M64
        assert osr.filter_e(ka, kb) == ((d >> 32) + 1) & M32
        a, b = osr.products(ka, kb)
        assert d == (a + b) & M64


def test_e_minus_the_digests_high_dword_is_0_1_or_2():
    seen, combos = set(), set()
    for ka, kb in PAIRS:
        cy, cy2, wrap = osr.carries(ka, kb)
        diff = (osr.filter_e(ka, kb) - (osr.open_full(ka, kb) >> 32)) & M32
        assert diff == 1 + cy - cy2
        seen.add(diff)
        combos.add((cy, cy2, wrap))
    assert seen == {0, 1, 2}
    assert len(combos) == 8                               # both carries and the wrap of a.hi + b.hi, in every combination


def test_fixed_operands():
    for ka in FIXED:
        for kb in FIXED:
            assert (ka, kb) in PAIRS[:36]
            e, h = osr.filter_e(ka, kb), osr.open_full(ka, kb)
            assert (e - (h >> 32)) & M32 in (0, 1, 2)
            assert e == (((((ka + kb) * osr.C) & M64) >> 32) + 1) & M32


def test_open_thr_saturates():
    assert osr.open_thr(0) == 2 and osr.open_thr(M32) == 2 and osr.open_thr(1 << 54) == (1 << 22) + 2
    assert osr.open_thr(0xFFFFFFFC_FFFFFFFF) == 0xFFFFFFFE
    for hi in (0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF):
        assert osr.open_thr(hi << 32) == osr.open_thr((hi << 32) | M32) == M32


def test_nothing_that_passes_is_filtered_out():
    digests = [(osr.open_full(ka, kb), osr.filter_e(ka, kb)) for ka, kb in PAIRS]
    for thr in THRESHOLDS:
        limit = osr.open_thr(thr)
        passing = at = above = 0
        for h, e in digests:
            if h <= thr:
                assert e <= limit, (hex(thr), hex(h), hex(e))
                passing += 1
                at += h == thr
            else:
                above += 1
        assert passing >= 400 and at >= 40                # digests below and AT the threshold ...
        assert above >= 40 or thr == M64                  # ... and above it, where there is an above
    # the test is not vacuous the other way: with thr.hi + 1 in place of thr.hi + 2 some passing digest is lost
    lost = sum(1 for thr in THRESHOLDS if thr >> 32 < 0xFFFFFFFD for h, e in digests if h <= thr and e > (thr >> 32) + 1)
    assert lost > 0
