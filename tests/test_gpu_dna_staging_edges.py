"""GPU parity of the rolling DNA kernel where a lane's run begins and ends, and of the lanes that stage the packed tile,
bit-exact against the C oracle with max_hash = 2^64 - 1 (every window's hash is compared; abundances are tracked, so a
window lost or hashed twice shows).

The launch picks the run length R by the size of the input: runs of 128 positions need at least cu_count * 1024 * 128
positions (2^25 on 256 CUs); a shorter input is walked in runs of 64 or 32.  The tests that are about a run of 128
therefore work on a FIELD: that many bases in device memory, 'N' everywhere except a few islands of valid mixed-case DNA
around the runs under test.  A window that holds an 'N' adds nothing (force = True), so the oracle is fed the islands
joined by one 'N' each -- the same windows; test_field_oracle_input checks that once against the whole field.  Only
the chunked bottom-num test uses plain inputs of a few tiles: its launches are chunks of 64 * num positions.

Runs under test: lanes 0, 1, 63, 64 and 511 of tile 0 and lane 0 of tile 1 (the edges of a wave and of the workgroup);
neighbouring runs share bases, so {0, 63, 511} and {1, 64, tile 1's 0} are edited in separate launches."""
import random

import pytest

pytestmark = pytest.mark.gpu

R = 128
TILE = 512 * R
MAXH = (1 << 64) - 1
KS = [21, 29, 30, 31, 32]
KCFG = KS + ["grouped31"]                         # the per-record-threshold kernel (two hashes per block) at k = 31
RUNSETS = [(0, 63 * R, 511 * R), (1 * R, 64 * R, TILE)]
ISLANDS = [(0, 1024), (62 * R, 67 * R), (509 * R, TILE + 3 * R)]
FAR_CUT = 1 << 20                                 # a record boundary among the 'N's, far from every island


def rand_dna(rng, n, lower=0.0):
    s = bytearray(rng.choice(b"ACGT") for _ in range(n))
    for i in range(n):
        if rng.random() < lower:
            s[i] |= 0x20
    return s


def same_state(g, o):
    assert g.mins == o.mins
    assert g.abunds == o.abunds


class Field:
    """`n` bases in device memory, the first one `shift` bytes past a 16-byte boundary"""

    def __init__(self, n, islands, tail, shift=0, seed=1, content=None):
        import torch
        self.torch = torch
        rng = random.Random(seed)
        self.n, self.shift = n, shift
        self.dev = torch.full((n + 64,), ord("N"), dtype=torch.uint8, device="cuda")
        assert self.dev.data_ptr() % 16 == 0
        self.base = {s: rand_dna(rng, e - s, lower=0.3) for s, e in islands}
        self.base.update(content or {})
        self.base[n - tail] = rand_dna(rng, tail, lower=0.3)          # the field ends in valid bases
        for s, d in self.base.items():
            self._write(s, d)
        torch.cuda.synchronize()

    def _write(self, s, data):
        t = self.torch
        self.dev[self.shift + s:self.shift + s + len(data)] = t.frombuffer(bytearray(data), dtype=t.uint8).to("cuda")

    def ptr(self):
        return self.dev.data_ptr() + self.shift

    def edited(self, edits):
        isl = {s: bytearray(d) for s, d in self.base.items()}
        touched = set()
        for pos, byte in edits:
            hit = [s for s, d in isl.items() if s <= pos < s + len(d)]
            assert len(hit) == 1, "edit outside the islands"
            isl[hit[0]][pos - hit[0]] = byte
            touched.add(hit[0])
        return isl, touched

    @staticmethod
    def records(isl, offs):
        """the oracle's input: per record, the pieces of the islands inside it, joined by one 'N'"""
        out = []
        for a, b in zip(offs, offs[1:]):
            pieces = [bytes(d[max(a, s) - s:min(b, s + len(d)) - s]) for s, d in sorted(isl.items()) if s < b and s + len(d) > a]
            out.append(b"N".join(pieces))
        return out

    def check(self, pkg, coracle, kcfg, edits=(), cuts=(), length=None, num=0):
        n = self.n if length is None else length
        isl, touched = self.edited(edits)
        if length is not None:                                           # a shorter field: the tail island is cut
            isl = {s: d[:max(0, n - s)] for s, d in isl.items() if s < n}
        try:
            for s in touched:
                self._write(s, isl[s])
            self.torch.cuda.synchronize()
            grouped = kcfg == "grouped31"
            offs = sorted(set([0, n] + [c for c in cuts if 0 < c < n] + ([FAR_CUT] if grouped else [])))
            recs = self.records(isl, offs)
            if grouped:
                # bottom-num sketches so large that every window is kept (the threshold of every record is 2^64 - 1)
                case = (n // 4 + 64, 31, False, 42, 0, False)
                gs = [pkg.KmerMinHash(*case) for _ in range(2)]
                os_ = [coracle.MinHash(*case) for _ in range(2)]
                groups = [i % 2 for i in range(len(recs))]
                pkg.KmerMinHash.add_sequences_grouped_dev(gs, self.ptr(), n, offs, groups, True)
                for r, grp in zip(recs, groups):
                    os_[grp].add_sequence(r, True)
                for g, o in zip(gs, os_):
                    assert g.mins == o.mins
            else:
                # num: a bottom-num sketch that the field does not fill (every window is kept all the same)
                case = (num, kcfg, False, 42, 0 if num else MAXH, True)
                g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
                g.add_sequences_dev(self.ptr(), n, offs, True)
                for r in recs:
                    o.add_sequence(r, True)
                assert len(o.mins) > 1000 and (not num or len(o.mins) < num)
                same_state(g, o)
        finally:
            for s in touched:
                self._write(s, self.base[s])


@pytest.fixture(scope="module")
def field_n():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 1024 * R + 2048 + 77


@pytest.fixture(scope="module")
def field(pkg, field_n):
    return Field(field_n, ISLANDS, tail=1024)


def test_field_oracle_input(pkg, coracle, field):
    """the islands joined by one 'N' give the oracle the same windows as the whole field"""
    whole = bytes(field.dev[field.shift:field.shift + field.n].cpu().numpy().tobytes())
    joined = Field.records(field.base, [0, field.n])[0]
    assert len(whole) == field.n and len(joined) < 10000
    for k in (21, 31):
        a, b = coracle.MinHash(0, k, False, 42, MAXH, True), coracle.MinHash(0, k, False, 42, MAXH, True)
        a.add_sequence(whole, True)
        b.add_sequence(joined, True)
        assert a.mins == b.mins and a.abunds == b.abunds and len(a.mins) > 1000
    field.check(pkg, coracle, 31)


def test_encode_every_byte_at_every_position(pkg, coracle, field_n):
    """1. Every byte value at each of the 16 positions of a staged chunk, between valid upper- and lower-case bases (valid
    bases inside a dirty dword), the device address of the first base 0...15 bytes past a 16-byte boundary.  The bytes
    fill the first four tiles of a field, so that they are staged for runs of 128 like everything else here."""
    rng = random.Random(16)
    blocks = []
    for v in range(256):
        for pos in range(16):
            blk = rand_dna(rng, 64, lower=0.4)
            blk[16 + pos] = v
            blocks.append(blk)
    rng.shuffle(blocks)
    seq = bytearray(b"".join(blocks))
    assert len(seq) == 4 * TILE
    for shift in range(16):
        f = Field(field_n, [], tail=256, shift=shift, content={0: seq})
        for k in (21, 31):
            f.check(pkg, coracle, k)
        del f


def edge_offsets(k):
    return list(range(k - 5, k + 4)) + list(range(R + k - 6, R + k + 3))


@pytest.mark.parametrize("kcfg", KCFG)
def test_bad_byte_at_run_edges(pkg, coracle, field, kcfg):
    """2. a byte other than ACGT at base offsets K-5 ... K+3 and R+K-6 ... R+K+2 from the start of a run"""
    k = 31 if kcfg == "grouped31" else kcfg
    for runs in RUNSETS:
        for off in edge_offsets(k):
            field.check(pkg, coracle, kcfg, edits=[(p + off, ord("N") if off % 2 else ord("x")) for p in runs])


@pytest.mark.parametrize("kcfg", KCFG)
def test_record_boundary_at_run_edges(pkg, coracle, field, kcfg):
    """2. a record boundary at the same offsets"""
    k = 31 if kcfg == "grouped31" else kcfg
    for runs in RUNSETS:
        for off in edge_offsets(k):
            field.check(pkg, coracle, kcfg, cuts=[p + off for p in runs])


@pytest.mark.parametrize("kcfg", KCFG)
def test_range_ends_inside_the_last_run(pkg, coracle, field, field_n, kcfg):
    """2. the range of positions ends at every offset inside the last run of 128 (nk < R): fields of every length
    n0 ... n0 + 127, whose last bases are valid"""
    n0 = field_n - 1024 + 300
    for j in range(R):
        field.check(pkg, coracle, kcfg, length=n0 + j)


@pytest.mark.parametrize("ksize", KS)
def test_chunked_ranges_end_inside_a_run(pkg, coracle, ksize):
    """2. ranges that end inside a run through the chunked bottom-num path (a sketch that the one-pass launch does not fill
    is built in chunks of max(65536, 64 * num) positions; launches of that size walk runs of 32): the last range ends at
    every offset of a run of 32, and num = 1037 ends the first range at 66368, in the middle of a run"""
    rng = random.Random(300 + ksize)
    unit = bytes(rand_dna(rng, 600))
    for num in (1500, 1037):
        for j in range(32):
            n = 200000 + j
            seq = (unit * (n // 600 + 1))[:n]
            case = (num, ksize, False, 42, 0, True)
            g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
            g.add_sequence(seq, True)
            o.add_sequence(seq, True)
            assert len(o.mins) < num                                  # the chunked path is the one taken
            same_state(g, o)


def dna_launches(pkg, fn):
    """rolling-kernel launches made while `fn` runs (as in tests/test_gpu_dna_kernel_edges.py)"""
    import ctypes as C
    L = pkg.lib()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    try:
        fn()
    finally:
        L.smh_profile_enable(0)
    ms, n = C.c_double(), C.c_uint64()
    L.smh_profile_get(b"dna_rolling", C.byref(ms), C.byref(n))
    return n.value


def test_chunked_range_ends_inside_a_run_of_128(pkg, coracle, field_n):
    """2. the same path with chunks long enough for runs of 128: num = field_n / 64 rounded to give chunks of
    cu_count * 1024 * 128 + 64 positions, so that the first range ends -- and the second begins -- 64 positions into a run,
    among valid bases whose windows must be counted exactly once.  (A chunk is a multiple of 64 positions: other offsets
    inside a run of 128 cannot be reached this way; the end of the input, above, reaches all of them.)"""
    num = (field_n - 2048 - 77) // 64 + 1
    c = 64 * num
    f = Field(2 * c + 3000, [(c - 700, c + 700)], tail=512, seed=3)
    for k in KS:
        assert dna_launches(pkg, lambda: f.check(pkg, coracle, k, num=num)) >= 3      # one-pass launch + ranged launches
        f.check(pkg, coracle, k, num=num, edits=[(c - 3, ord("N")), (c + k + 1, ord("n"))])
        f.check(pkg, coracle, k, num=num, cuts=[c - 2, c + 5])


@pytest.mark.parametrize("kcfg", KCFG)
def test_bad_byte_in_the_warm_up(pkg, coracle, field, kcfg):
    """3. a byte other than ACGT at each of the offsets 0 ... 29 of a run"""
    for runs in RUNSETS:
        for off in range(30):
            field.check(pkg, coracle, kcfg, edits=[(p + off, ord("n") if off % 2 else ord("R")) for p in runs])


@pytest.mark.parametrize("kcfg", KCFG)
def test_record_starts_in_the_warm_up(pkg, coracle, field, kcfg):
    """3. a record starts at each of the offsets 0 ... 29 of a run"""
    for runs in RUNSETS:
        for off in range(30):
            field.check(pkg, coracle, kcfg, cuts=[p + off for p in runs])


def test_shifted_field(pkg, coracle, field_n):
    """the run edges and the warm-up once more with the first base 5 bytes past a 16-byte boundary (the packed tile's
    shift within its first code dword is not zero), k = 31, both kernels"""
    f = Field(field_n, ISLANDS, tail=1024, shift=5, seed=2)
    for kcfg in (31, "grouped31"):
        for runs in RUNSETS:
            for off in list(range(0, 30, 3)) + edge_offsets(31)[::2]:
                f.check(pkg, coracle, kcfg, edits=[(p + off, ord("N")) for p in runs])
                f.check(pkg, coracle, kcfg, cuts=[p + off for p in runs])
