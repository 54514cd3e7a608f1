"""The lanes that stage the packed tile of the rolling DNA kernel decide per 16 input bytes whether all are ACGT in either
case: the 2-bit code comes from bits 1..2 of a byte, the byte is rebuilt from the code, and the difference must be zero
outside bit 5 (the case bit).  Where bit 5 is masked is free; a mask in the wrong place, or a wider one, would accept bytes
that differ from a valid letter in ONE bit.  The inputs here hold only such bytes besides valid mixed-case DNA:

    '!' 0x21 = 'a' ^ 0x40      '`' 0x60 = 'a' ^ 0x01      0x01 = 'A' ^ 0x40
    'Q' 0x51 = 'A' ^ 0x10      0xF4 = 't' ^ 0x80           'E' 0x45 = 'A' ^ 0x04 (bit 2: the code changes too)

each at every one of the 16 positions of a staged chunk, in the chunk that straddles the boundary between two lanes' runs
(the first base 5 bytes past a 16-byte boundary, so that no run begins on a chunk), and in the last, partly filled chunk
of the buffer.  k = 31 and k = 21, bit-exact against the C oracle with max_hash = 2^64 - 1 and abundances: a byte taken
for a base adds windows that the oracle does not have.  force = False must stop at the same k-mer with the same message
(0xF4 is not UTF-8: there the reference panics while it builds the message, and both sides must report that).

Inputs of a few KB are walked in runs of 32; the straddling chunk is checked once more on a field long enough for the
runs of 128 that the benchmark has (islands of DNA in 'N', as in tests/test_gpu_dna_staging_edges.py), force = True
only: with force = False such a field stops at its first 'N'."""
import random

import pytest

pytestmark = pytest.mark.gpu

MAXH = (1 << 64) - 1
NEAR = [0x21, 0x60, 0x01, 0x51, 0xF4, 0x45]
KS = [31, 21]
SHIFTS = [0, 5]


def rand_dna(rng, n):
    return bytearray(rng.choice(b"ACGTacgt") for _ in range(n))


def blocks_input(rng, tail_byte):
    """64-byte blocks of valid bases, each near-letter at each of the 16 offsets of the block's second chunk; then a tail
    whose last, partly filled chunk holds `tail_byte` three bases before the end"""
    blocks = []
    for v in NEAR:
        for pos in range(16):
            blk = rand_dna(rng, 64)
            blk[16 + pos] = v
            blocks.append(blk)
    rng.shuffle(blocks)
    seq = bytearray(b"".join(blocks)) + rand_dna(rng, 16 * 6 + 7)
    seq[-3] = tail_byte
    return seq


class DevBuf:
    def __init__(self, nbytes):
        import torch
        self.torch = torch
        self.t = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0

    def put(self, shift, data, at=0):
        t = self.torch
        self.t[shift + at:shift + at + len(data)] = t.frombuffer(bytearray(data), dtype=t.uint8).to("cuda")
        t.cuda.synchronize()
        return self.t.data_ptr() + shift


@pytest.fixture(scope="module")
def small(pkg):
    return DevBuf(8192)


def run_both(pkg, coracle, k, ptr, host, force):
    """the GPU sketch of the device bytes and the oracle's of the host bytes; with force = False both must fail alike"""
    case = (0, k, False, 42, MAXH, True)
    g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
    if force:
        g.add_sequences_dev(ptr, len(host), [0, len(host)], True)
        o.add_sequence(bytes(host), True)
    else:
        with pytest.raises(coracle.OracleError) as eo:
            o.add_sequence(bytes(host), False)
        with pytest.raises(pkg.SourmashError) as eg:
            g.add_sequences_dev(ptr, len(host), [0, len(host)], False)
        if any(c > 0x7f for c in host):
            # the k-mer of the message is not UTF-8: the reference panics where it builds the message (status 1)
            assert eo.value.code == 1 and eg.value.code == 1
        else:
            assert eo.value.code == 1101 and len(eo.value.message) == k
            assert eg.value.code == 1101 and eg.value.message.endswith(eo.value.message)
    assert g.mins == o.mins
    assert g.abunds == o.abunds
    return o


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("k", KS)
def test_near_letters_at_every_chunk_position(k, shift, small, pkg, coracle):
    """force = True: all six bytes at all 16 positions, and one in the last chunk, in one input per tail byte"""
    for i, tail in enumerate(NEAR):
        seq = blocks_input(random.Random(500 + i), tail)
        o = run_both(pkg, coracle, k, small.put(shift, seq), seq, True)
        assert len(o.mins) > 1000


def test_valid_letters_in_either_case(small, pkg, coracle):
    """a c g t and A C G T alone: nothing is dirty, every window is hashed"""
    rng = random.Random(7)
    seq = bytearray(b"acgtACGT" * 4) + rand_dna(rng, 3000)
    for k in KS:
        for shift in SHIFTS:
            for force in (True, False):
                case = (0, k, False, 42, MAXH, True)
                g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
                g.add_sequences_dev(small.put(shift, seq), len(seq), [0, len(seq)], force)
                o.add_sequence(bytes(seq), force)
                assert sum(o.abunds) == len(seq) - k + 1
                assert g.mins == o.mins and g.abunds == o.abunds


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("k", KS)
def test_error_kmer_without_force(k, shift, small, pkg, coracle):
    """force = False: one near-letter per input, at each of the 16 positions of a chunk (six bytes, 16 positions), in the
    chunk that straddles a run boundary (shift 5: bases 123 ... 138 around base 128 = 4 runs of 32) and in the last,
    partly filled chunk"""
    rng = random.Random(900 + k + shift)
    base = rand_dna(rng, 16 * 20 + 9)
    n = len(base)
    for v in NEAR:
        for at in list(range(128, 144)) + [n - 3]:
            seq = bytearray(base)
            seq[at] = v
            run_both(pkg, coracle, k, small.put(shift, seq), seq, False)


def test_straddling_chunk_in_runs_of_128(pkg, coracle):
    """runs of 128 need cu_count * 1024 * 128 positions.  A field of 'N' with one island of DNA around the boundary between
    the runs of lanes 1 and 2 of the first tile (base 256), the first base 5 bytes past a 16-byte boundary: the chunk of
    bases 251 ... 266 straddles it.  Each near-letter on either side of the boundary."""
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count * 1024 * 128 + 2048 + 77
    buf = torch.full((n + 64,), ord("N"), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    shift, lo, hi = 5, 128, 400
    rng = random.Random(11)
    island, tail = rand_dna(rng, hi - lo), rand_dna(rng, 100)

    def put(at, data):
        buf[shift + at:shift + at + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")

    put(n - len(tail), tail)                                          # the field ends in valid bases
    for k in KS:
        for j, v in enumerate(NEAR):
            isl = bytearray(island)
            isl[(251 + j) - lo] = v                                   # 251 ... 256: both sides of base 256
            isl[(266 - j) - lo] = NEAR[(j + 1) % len(NEAR)]           # 266 ... 261
            put(lo, isl)
            torch.cuda.synchronize()
            case = (0, k, False, 42, MAXH, True)
            g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
            g.add_sequences_dev(buf.data_ptr() + shift, n, [0, n], True)
            o.add_sequence(bytes(isl) + b"N" + bytes(tail), True)      # the same windows: an 'N' ends every other one
            assert len(o.mins) > 100
            assert g.mins == o.mins and g.abunds == o.abunds
