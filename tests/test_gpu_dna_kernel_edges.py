"""GPU parity of the rolling DNA kernel at the edges of its per-group and per-run bookkeeping, bit-exact against the
C oracle: runs that end inside a group of four bases, every (k-1) mod 4 on the two-limb path (k = 29..32, and the
compile-time k = 21 and 31), record boundaries and non-ACGT bytes in the first and last group of a lane's run,
lowercase input, chunked (ranged) launches that do not start on a tile boundary (from host memory and from odd device
addresses), and batches smaller than one tile."""
import random

import pytest

pytestmark = pytest.mark.gpu

KS = [21, 29, 30, 31, 32]


def same_state(g, o):
    assert g.mins == o.mins
    assert g.abunds == o.abunds


def rand_dna(rng, n, lower=0.0):
    s = bytearray(rng.choice(b"ACGT") for _ in range(n))
    if lower:
        for i in range(n):
            if rng.random() < lower:
                s[i] |= 0x20
    return bytes(s)


def with_bad_bytes(rng, seq, run=128):
    """non-ACGT bytes in the first and the last group of several lane runs (runs are `run` bases apart)"""
    s = bytearray(seq)
    for r0 in range(run, len(s) - run, run * 7):
        for off in (0, 1, 3, run - 4, run - 2, run - 1):
            if rng.random() < 0.5 and r0 + off < len(s):
                s[r0 + off] = rng.choice(b"NnRX")
    return bytes(s)


def check(pkg, coracle, recs, ksize, num=0, max_hash=(1 << 64) // 20, force=True, batch=True):
    case = (num, ksize, False, 42, max_hash, True)
    g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
    if batch:
        g.add_sequences(recs, force)
    else:
        for r in recs:
            g.add_sequence(r, force)
    for r in recs:
        o.add_sequence(r, force)
    same_state(g, o)


@pytest.mark.parametrize("ksize", KS)
def test_run_ends_inside_a_group(pkg, coracle, ksize):
    # lengths around multiples of the lane run and of four, so that the last window of a lane's run ends at every
    # offset inside its group of four
    rng = random.Random(ksize)
    for n in [ksize, ksize + 1, ksize + 2, ksize + 3, 127 + ksize, 128 + ksize, 129 + ksize, 130 + ksize,
              4096 + ksize - 1, 65536 + ksize - 3, 65536 * 2 + 5]:
        check(pkg, coracle, [rand_dna(rng, n)], ksize)


@pytest.mark.parametrize("ksize", KS)
def test_bad_bytes_and_records_at_run_edges(pkg, coracle, ksize):
    rng = random.Random(100 + ksize)
    big = with_bad_bytes(rng, rand_dna(rng, 300000, lower=0.05))
    check(pkg, coracle, [big], ksize)
    # records whose boundaries fall in the first / last group of a lane's run
    recs = []
    for n in [128 * 3 + 1, 128 * 5 - 1, 128 * 2 + 2, 128 - 3, 128 * 9 + 4, 128 * 4, ksize - 1, ksize, 128 * 11 + 3]:
        recs.append(with_bad_bytes(rng, rand_dna(rng, n, lower=0.1), 128))
    recs = recs * 40
    check(pkg, coracle, recs, ksize)


@pytest.mark.parametrize("ksize", [29, 31, 32])
def test_lowercase(pkg, coracle, ksize):
    rng = random.Random(7 + ksize)
    check(pkg, coracle, [rand_dna(rng, 70000).lower(), rand_dna(rng, 70000, lower=0.5)], ksize)


def low_complexity(rng, n, unit=600, boundary=0):
    """`n` bases repeating one random unit of `unit` bases: fewer distinct k-mers than a bottom-num sketch of 1037 or 1500
    holds, so the sketch is not settled by the one-pass launch and is built chunk by chunk.  A few substitutions, non-ACGT
    bytes and lowercase letters sit around `boundary` (a chunk boundary)."""
    u = rand_dna(rng, unit)
    s = bytearray((u * (n // unit + 1))[:n])
    for off in range(-40, 40, 7):
        i = boundary + off
        if 0 <= i < n:
            s[i] = rng.choice(b"ACGTNacgtn")
    for i in range(max(0, boundary - 3), min(n, boundary + 3)):
        s[i] |= 0x20 if s[i] in b"ACGT" else 0
    return bytes(s)


def dna_launches(pkg, g, fn):
    """rolling-kernel launches made while `fn` adds to `g` and the sketch is read back (add_sequence only queues the record:
    the hashing runs when the state is asked for)"""
    import ctypes as C
    L = pkg.lib()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    try:
        fn()
        g.mins
    finally:
        L.smh_profile_enable(0)
    ms, n = C.c_double(), C.c_uint64()
    L.smh_profile_get(b"dna_rolling", C.byref(ms), C.byref(n))
    return n.value


@pytest.mark.parametrize("ksize", [21, 30, 31])
def test_ranged_launches(pkg, coracle, ksize):
    # A bottom-num sketch whose input has fewer distinct k-mers than num is hashed in chunks of max(65536, 64 * num)
    # positions: num = 1500 starts the second launch at position 96000, num = 1037 at 66368 -- neither a tile boundary.
    # Abundances are tracked, so a window lost or hashed twice at a range boundary shows.  Through an odd device pointer
    # every tile also starts off a 16-byte boundary (the packed tile's shift within its first code dword is not zero).
    import torch
    rng = random.Random(55 + ksize)
    for num in (1500, 1037):
        chunk = max(65536, 64 * num)
        seq = low_complexity(rng, 400003, boundary=chunk)
        case = (num, ksize, False, 42, 0, True)
        o = coracle.MinHash(*case)
        o.add_sequence(seq, True)
        assert len(o.mins) < num                                  # the chunked path is the one taken
        g = pkg.KmerMinHash(*case)
        assert dna_launches(pkg, g, lambda: g.add_sequence(seq, True)) >= 3      # one-pass launch + two ranged launches
        same_state(g, o)
        for shift in (5, 7):
            buf = torch.zeros(len(seq) + 16, dtype=torch.uint8, device="cuda")
            buf[shift:shift + len(seq)] = torch.frombuffer(bytearray(seq), dtype=torch.uint8).to("cuda")
            torch.cuda.synchronize()
            g = pkg.KmerMinHash(*case)
            assert dna_launches(pkg, g, lambda: g.add_sequences_dev(buf.data_ptr() + shift, len(seq), [0, len(seq)], True)) >= 3
            same_state(g, o)


@pytest.mark.parametrize("ksize", KS)
def test_batch_smaller_than_a_tile(pkg, coracle, ksize):
    rng = random.Random(900 + ksize)
    for n in [ksize, ksize + 5, 200, 1000, 4099]:
        check(pkg, coracle, [rand_dna(rng, n, lower=0.1)], ksize, max_hash=(1 << 64) - 1)
    check(pkg, coracle, [rand_dna(rng, n) for n in (ksize - 1, ksize, 40, 3, 130)], ksize, max_hash=(1 << 64) - 1)
