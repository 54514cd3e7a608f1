"""The folded tables of the DNA kernel's k2 words with the high dword's cross term taken from the tables, restated in
Python integers: low-half entries {T2'', a.hi}, high-half entries {B, B'}, and the three-instruction mix
S = a.hi + B; p = S * lo32(2 c1) + T2''; p.hi += B'.  Checked against rotl(W * c2, 33) * c1 for every low half x every
high half of 4, 3, 2 and 1 letters (87 040 words) and for the low half alone (256 words, the high half reads the zero
entry).  No GPU needed."""

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
C1 = 0x87C37B91114253D5
C2 = 0x4CF5AD432745937F
C1X2 = (2 * C1) & M64
CL, CH = C1X2 & M32, C1X2 >> 32


def letters(idx, nb):
    """the table index's nb 2-bit digits as ASCII bytes, first letter in the low byte (as the kernel builds them)"""
    v = 0
    for j in range(nb):
        v |= b"ACGT"[(idx >> (2 * j)) & 3] << (8 * j)
    return v


def rotl64(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def mix_k2(w):
    return (rotl64((w * C2) & M64, 33) * C1) & M64


def low_entry(v):
    """{T2'', a.hi} of a k2 word's low half"""
    prod = (v * C2) & M64
    m, ahi = prod & M32, prod >> 32
    t2 = ((((m >> 31) | ((m & 0x7FFFFFFF) << 33)) & M64) * C1) & M64
    return (t2 + (((ahi * CH) & M32) << 32)) & M64, ahi


def high_entry(v):
    """{B, B'} of a k2 word's high half"""
    b = (v * C2) & M32
    return b, (b * CH) & M32


def mix_from_entries(lo, hi):
    t, ahi = lo
    b, bp = hi
    s = (ahi + b) & M32                                   # v_add_u32
    p = (s * CL + t) & M64                                # v_mad_u64_u32
    return (p & M32) | ((((p >> 32) + bp) & M32) << 32)   # v_add_u32 on the high dword


LOW = [(letters(i, 4), low_entry(letters(i, 4))) for i in range(256)]


def test_zero_entries():
    assert low_entry(0) == (0, 0) and high_entry(0) == (0, 0)
    assert mix_from_entries((0, 0), (0, 0)) == 0 == mix_k2(0)


def test_low_half_alone():
    n = 0
    for v, lo in LOW:
        assert mix_from_entries(lo, (0, 0)) == mix_k2(v)
        n += 1
    # a partial low half (the k-mer ends inside it: run-time k = 25, 26, 27)
    for nb in (1, 2, 3):
        for i in range(4 ** nb):
            v = letters(i, nb)
            assert mix_from_entries(low_entry(v), (0, 0)) == mix_k2(v)
    assert n == 256


def test_every_low_half_with_every_high_half():
    words = wraps = 0
    for nb in (4, 3, 2, 1):
        highs = [(letters(i, nb), high_entry(letters(i, nb))) for i in range(4 ** nb)]
        for vl, lo in LOW:
            for vh, hi in highs:
                assert mix_from_entries(lo, hi) == mix_k2(vl | (vh << 32))
                words += 1
                wraps += lo[1] + hi[0] > M32
    assert words == 256 * (256 + 64 + 16 + 4) == 87040
    assert wraps == 42897                                  # words whose a.hi + B wraps: the wrap drops out (2^32 * ch == 0 mod 2^32)
