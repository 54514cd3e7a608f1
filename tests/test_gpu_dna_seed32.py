"""The rolling DNA kernel's variant for seeds below 2^32 (k_dna_rolling's S32: the seed's high dword is never read) against
the C oracle, and the launcher's choice between it and the unchanged kernel.

The packed two-limb kernels with a launch-uniform threshold -- k = 31 (the bench kernel), k = 21 and the run-time-k kernel
(k = 29, 32 here) -- take the variant when seed < 2^32 and the code they always had otherwise; k = 51 (four limbs) and the
per-record kernel of grouped bottom-num batches have no such variant.  Every case asserts through the launch counters
dna_seed32 / dna_seed64 which one ran.

One input of five records (one too short at k = 31, two at k = 32 and 51, one with an 'N'), force = True.  With
max_hash = 2^64 - 1 every window is kept, so one wrong hash shows; scaled = 1000 with abundances runs the same kernels
with the filter that the benchmark uses.  A build that takes the variant for every seed fails every case with a seed at
or above 2^32 on the two-limb kernels (24 of the 62 cases) and no other."""
import ctypes as C
import random

import pytest

pytestmark = pytest.mark.gpu

MAXH = (1 << 64) - 1
SCALED = (1 << 64) // 1000
SEEDS = [0, 42, (1 << 32) - 1, 1 << 32, (1 << 32) + 42, (1 << 63) + 5]
KS = [31, 21, 29, 32, 51]


def _records():
    rng = random.Random(1132)

    def dna(n, lower=0.0):
        return bytearray(rng.choice(b"acgt" if rng.random() < lower else b"ACGT") for _ in range(n))

    with_n = dna(300)
    with_n[150] = ord("N")
    return [bytes(r) for r in (dna(700, lower=0.4), dna(31), dna(30), with_n, dna(2000))]


RECORDS = _records()


def _counts(pkg):
    out = []
    for name in ("dna_seed32", "dna_seed64"):
        ms, n = C.c_double(), C.c_uint64()
        pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(n))
        out.append(n.value)
    return tuple(out)


def _expect_variant(counts, seed32):
    s32, s64 = counts
    print("dna_seed32 launches", s32, "dna_seed64 launches", s64)
    if seed32:
        assert s32 >= 1 and s64 == 0
    else:
        assert s64 >= 1 and s32 == 0


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("max_hash", [MAXH, SCALED], ids=["every_window", "scaled1000"])
def test_sketch_matches_oracle(k, seed, max_hash, pkg, coracle):
    case = (0, k, False, seed, max_hash, True)
    g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
    pkg.lib().smh_profile_reset()
    g.add_sequences(RECORDS, True)
    counts = _counts(pkg)
    for r in RECORDS:
        o.add_sequence(r, True)
    windows = sum(max(len(r) - k + 1, 0) for r in RECORDS) - k      # the 'N' costs k windows
    if max_hash == MAXH:
        assert sum(o.abunds) == windows and len(o.mins) > 2000
    assert g.mins == o.mins
    assert g.abunds == o.abunds
    _expect_variant(counts, seed < (1 << 32) and k <= 32)


@pytest.mark.parametrize("seed", [42, (1 << 32) + 42])
def test_grouped_bottom_num_keeps_its_kernel(seed, pkg, coracle):
    """a grouped bottom-num batch runs the per-record kernel, which has no variant: dna_seed64 for either seed"""
    case = (500, 31, False, seed, 0, False)
    groups = [0, 1, 1, 0, 1]
    gs, os_ = [pkg.KmerMinHash(*case) for _ in range(2)], [coracle.MinHash(*case) for _ in range(2)]
    pkg.lib().smh_profile_reset()
    pkg.KmerMinHash.add_sequences_grouped(gs, RECORDS, groups, True)
    counts = _counts(pkg)
    for r, grp in zip(RECORDS, groups):
        os_[grp].add_sequence(r, True)
    for g, o in zip(gs, os_):
        assert len(o.mins) == 500
        assert g.mins == o.mins
    _expect_variant(counts, False)
