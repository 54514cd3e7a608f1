"""The sketch kernels' filter on the open digest, restated in Python integers (murmur_device.hpp: w2_fmix_pre,
open_hi_sum1<true>, open_thr<true>, open_full).  murmur64 of a string is h = fmix(h1) + fmix(h2); the kernels stop each
fmix in front of its last multiply, ka = pre(h1), kb = pre(h2), and test E = hi32((ka + kb) * C) + 1 against
open_thr(thr) before they form a = ka * C, b = kb * C and h = (a ^ a >> 33) + (b ^ b >> 33).
No product import; tests/test_open_sum_identity.py checks this file, the GPU test classifies its inputs with it."""
import pyoracle

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
C = 0xC4CEB9FE1A85EC53                    # fmix's second constant
CL, CH = C & M32, C >> 32
C_INV = pow(C, -1, 1 << 64)
FMIX_C1 = 0xFF51AFD7ED558CCD


def filter_e(ka, kb):
    """E as the kernel forms it, instruction by instruction"""
    s = (ka + kb) & M64                                   # v_lshl_add_u64 (the operands stay)
    s_lo, s_hi = s & M32, s >> 32
    s0 = s_hi * CL + 1                                    # v_mad_u64_u32, addend 1: a 64-bit result
    s1 = (s_lo * CH + s0) & M64                           # v_mad_u64_u32, addend s0 (mod 2^64); only its low dword is used
    m = (s_lo * CL) >> 32                                 # v_mul_hi_u32
    return ((s1 & M32) + m) & M32                         # v_add_u32


def open_thr(thr):
    hi = thr >> 32
    return M32 if hi >= 0xFFFFFFFD else hi + 2


def products(ka, kb):
    return (ka * C) & M64, (kb * C) & M64


def open_full(ka, kb):
    a, b = products(ka, kb)
    return ((a ^ (a >> 33)) + (b ^ (b >> 33))) & M64


def carries(ka, kb):
    """(cy, cy', wrap): the carries of a.lo + b.lo and of the xor-shifted low dwords, and whether a.hi + b.hi wraps"""
    a, b = products(ka, kb)
    al, bl = a & M32, b & M32
    cy = (al + bl) >> 32
    cy2 = (((a ^ (a >> 33)) & M32) + ((b ^ (b >> 33)) & M32)) >> 32
    return cy, cy2, ((a >> 32) + (b >> 32)) >> 32


def pair_from_products(a, b):
    """(ka, kb) whose products are a and b: C is odd, so x -> x * C is a bijection of the 64-bit integers"""
    return (a * C_INV) & M64, (b * C_INV) & M64


def pair_with_digest(h, a_shifted):
    """(ka, kb) with open_full(ka, kb) == h whose first xor-shifted product is a_shifted"""
    b_shifted = (h - a_shifted) & M64
    undo = lambda x: x ^ (x >> 33)                        # k ^= k >> 33 is its own inverse (33 >= 32)
    return pair_from_products(undo(a_shifted), undo(b_shifted))


def pre(h):
    """fmix64 up to, not including, its last multiply"""
    h ^= h >> 33
    h = (h * FMIX_C1) & M64
    return h ^ (h >> 33)


def murmur_pre(data, seed=42):
    """(ka, kb) of murmur3_x64_128's first word: pyoracle.murmur3_x64_128 up to the fmix calls"""
    data = bytes(data)
    n = len(data)
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M64
    h1 = h2 = seed & M64
    full = n - (n % 16)
    for off in range(0, full, 16):
        k1 = int.from_bytes(data[off:off + 8], "little")
        k2 = int.from_bytes(data[off + 8:off + 16], "little")
        h1 ^= (rotl((k1 * pyoracle.C1) & M64, 31) * pyoracle.C2) & M64
        h1 = ((rotl(h1, 27) + h2) * 5 + 0x52DCE729) & M64
        h2 ^= (rotl((k2 * pyoracle.C2) & M64, 33) * pyoracle.C1) & M64
        h2 = ((rotl(h2, 31) + h1) * 5 + 0x38495AB5) & M64
    tail = data[full:]
    if len(tail) > 8:
        h2 ^= (rotl((int.from_bytes(tail[8:], "little") * pyoracle.C2) & M64, 33) * pyoracle.C1) & M64
    if len(tail) > 0:
        h1 ^= (rotl((int.from_bytes(tail[:8], "little") * pyoracle.C1) & M64, 31) * pyoracle.C2) & M64
    h1 ^= n
    h2 ^= n
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    return pre(h1), pre(h2)


def classify(word, seed=42):
    """(h, E - h.hi mod 2^32) of a hashed string; h is asserted equal to the oracle's murmur"""
    ka, kb = murmur_pre(word, seed)
    h = open_full(ka, kb)
    assert h == pyoracle.hash_murmur(word, seed)
    return h, (filter_e(ka, kb) - (h >> 32)) & M32
