"""GPU parity of the one-pass protein kernel (k_protein_fused + k_spliced_windows + k_protein_positions) where a lane's run
begins and ends, window by window and bit-exact against the C oracle: max_hash = 2^64 - 1 with abundances, or a
bottom-num sketch larger than the number of windows, so that a window lost or hashed twice shows.

launch_protein_fused picks the run length R by the size of the input: runs of 128 window starts need
len >> 7 >= cu_count * 1024 (32 MiB on 256 CUs), runs of 64 half of that, anything shorter walks runs of 32.  The tests
about R = 128 and R = 64 therefore work on a FIELD (tests/protein_restatement.py): that many bases in device memory cut
into records -- valid DNA in records of 16 bases, shorter than every ksize here, which add nothing (src/lib.rs:257;
tests/test_protein_field_rules.py) and none of whose spans reaches the slow list (every span in them starts in an
"earlier record") -- and a few ISLANDS, records of mixed-case DNA around the runs under test.  The oracle is fed the island
records only.  A field of 'N' would not do here: every unclean span goes to k_spliced_windows and would overflow its
list, and dropped codons splice islands together (quirk Q8).

Runs under test: lanes 0, 1, 63, 64 and 511 of tile 0 and lane 0 of tile 1 (the edges of a wave and of the workgroup).  A
run's window starts are [p0, p0 + R), p0 = lane * R; the lane walks bases [p0, p0 + R + 3W - 1).  Neighbouring runs share
bases, so {0, 63, 511} and {1, 64, tile 1's 0} are edited in separate launches.  Window lengths W = 7, 9, 10 (ksize 21, 27,
30); W = 9 has k2 tables of its own.

Every check asserts its route (the fused launch ran, k_translate and k_hash_windows did not) and a floor on the oracle's
number of distinct windows, half of what the oracle gives for the unedited islands (MEASURED, on the CPU)."""
import random

import numpy as np
import pytest

import protein_restatement as pr

pytestmark = pytest.mark.gpu

MAXH = (1 << 64) - 1
KSIZES = [21, 27, 30]
# distinct windows the oracle reports for the unedited island records, measured on the CPU with the oracle alone
# ((R, ksize): count; R = 32 is the plain input of test_runs_of_32); every assertion takes half as its floor
MEASURED = {(128, 21): 12319, (128, 27): 12259, (128, 30): 12229, (64, 21): 7239, (64, 27): 7191, (64, 30): 7167,
            (32, 21): 3600, (32, 27): 3552, (32, 30): 3528}


def run_starts(R):
    """the two sets of runs under test"""
    return [(0, 63 * R, 511 * R), (R, 64 * R, 512 * R)]


def edge_offsets(W, R):
    near = [-1, 0, 1, 3 * W - 2, 3 * W - 1, 3 * W]
    return near + [R + x for x in near]


def layout(cu):
    """(n128, n64, islands) for a device of `cu` compute units: the R = 128 field, the length of its R = 64 prefix (which
    ends inside the island around the half-way mark) and the islands -- the runs under test for both run lengths, the
    half-way mark, and the end of the field"""
    tail0 = cu * 1024 * 128
    half = cu * 1024 * 64
    n128 = tail0 + 2048 + 77
    islands = [(0, 1024), (3840, 4480), (7808, 8576), (32512, 33024), (65152, 65920),
               (half - 256, half + 1024), (tail0 + 256, n128)]
    return n128, half + 333, islands


def island_bytes(islands):
    """the islands' content (a function of their order and sizes only).  The second island holds a stretch, 40 other bases
    and the stretch's reverse complement; the third begins with the same stretch: hashes repeat within a record across
    strands and across records, which is what makes a small tracked bottom-num sketch depend on the order (quirk Q3)"""
    rng = random.Random(20)
    isl = {s: pr.rand_dna(rng, e - s, lower=0.3) for s, e in islands}
    x = bytes(isl[islands[1][0]][:300]).upper()
    rc = x[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))
    isl[islands[1][0]][340:640] = rc
    isl[islands[2][0]][:300] = x
    return isl


class Field:
    """the field in device memory, its first base `shift` bytes past a 16-byte boundary"""

    def __init__(self, cu, shift=0):
        import torch
        self.torch = torch
        self.n128, self.n64, self.islands = layout(cu)
        self.shift = shift
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7 + shift)
        lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
        self.dev = lut[torch.randint(0, 4, (self.n128 + 80,), device="cuda", generator=gen)]   # bases past the end are valid too
        assert self.dev.data_ptr() % 16 == 0
        self.base = island_bytes(self.islands)
        for s, d in self.base.items():
            self._write(s, d)
        torch.cuda.synchronize()
        self.off = pr.field_offsets(self.n128, self.islands)

    def _write(self, s, data):
        t = self.torch
        self.dev[self.shift + s:self.shift + s + len(data)] = t.frombuffer(bytearray(data), dtype=t.uint8).to("cuda")

    def ptr(self):
        return self.dev.data_ptr() + self.shift

    def check(self, pkg, coracle, ksize, R=128, mode="scaled", edits=(), cuts=(), length=None, num=0):
        """sketch the first `length` bases (default: the whole field for R = 128, the prefix for R = 64) with `edits`
        [(position, byte)] written into the islands and `cuts` added as record boundaries; compare with the oracle on the
        island records"""
        n = length if length is not None else (self.n128 if R == 128 else self.n64)
        # the launch's run length, by the rule of launch_protein_fused
        cu = (self.n128 - 2048 - 77) // (1024 * 128)
        assert (n >> 7 >= cu * 1024) == (R == 128) and n >> 6 >= cu * 1024
        isl = {s: bytearray(d) for s, d in self.base.items()}
        touched = set()
        for pos, byte in edits:
            hit = [s for s, d in isl.items() if s <= pos < s + len(d)]
            assert len(hit) == 1, "edit outside the islands"
            isl[hit[0]][pos - hit[0]] = byte
            touched.add(hit[0])
        cuts = [c for c in cuts if 0 < c < n]
        for c in cuts:
            assert any(s < c < s + len(d) for s, d in isl.items()), "cut outside the islands"
        off = pr.with_cuts(pr.prefix_offsets(self.off, n), cuts)
        recs = pr.island_records(isl, cuts, n)
        floor = MEASURED[(R, ksize)] // 2
        try:
            for s in touched:
                self._write(s, isl[s])
            self.torch.cuda.synchronize()
            if mode == "grouped":
                # the island records alternate between two scaled sketches (the filler records feed the first)
                case = (0, ksize, True, 42, MAXH, True)
                gs = [pkg.KmerMinHash(*case) for _ in range(2)]
                os_ = [coracle.MinHash(*case) for _ in range(2)]
                grp = np.zeros(len(off) - 1, dtype=np.uint32)
                for i, (s, r) in enumerate(recs):
                    at = int(np.searchsorted(off, np.uint64(s)))
                    assert int(off[at]) == s and int(off[at + 1]) == s + len(r)
                    grp[at] = i % 2
                    os_[i % 2].add_sequence(r, True)
                c = pr.route_counters(pkg, lambda: pkg.KmerMinHash.add_sequences_grouped_dev(gs, self.ptr(), n, off, grp, True))
                assert sum(len(o.mins) for o in os_) >= floor and min(len(o.mins) for o in os_) >= floor // 8
                for g, o in zip(gs, os_):
                    pr.same_state(g, o)
            else:
                case = (num, ksize, True, 42, 0 if num else MAXH, True)
                g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
                c = pr.route_counters(pkg, lambda: g.add_sequences_dev(self.ptr(), n, off, True))
                for _, r in recs:
                    o.add_sequence(r, True)
                if mode != "small_num":
                    assert len(o.mins) >= floor and (not num or len(o.mins) < num)
                pr.same_state(g, o)
            assert c["protein_fused"] >= 1 and c["translate"] == 0 and c["hash_windows"] == 0, c
            return o if mode != "grouped" else os_
        finally:
            for s in touched:
                self._write(s, self.base[s])


@pytest.fixture(scope="module")
def cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def field(pkg, cu):
    return Field(cu)


@pytest.mark.parametrize("R", [128, 64])
@pytest.mark.parametrize("ksize", KSIZES)
def test_bad_byte_at_run_edges(pkg, coracle, field, ksize, R):
    """an 'N' at base p0 - 1, p0, p0 + 1, p0 + 3W - 2, p0 + 3W - 1, p0 + 3W and at the same offsets from p0 + R: the windows
    that splice over the dropped codon come from k_spliced_windows, each exactly once, the clean ones from the fused
    kernel, each exactly once; and runs of 4 and of 7 'N's that straddle the first and the last window start of a run"""
    W = ksize // 3
    for runs in run_starts(R):
        for off in edge_offsets(W, R):
            field.check(pkg, coracle, ksize, R, edits=[(p + off, ord("N")) for p in runs if p + off >= 0])
        for ln, at in ((4, -2), (7, -3), (4, R - 2), (7, R - 3), (7, 3 * W - 4), (4, R + 3 * W - 3)):
            field.check(pkg, coracle, ksize, R, edits=[(p + at + i, ord("N")) for p in runs for i in range(ln) if p + at + i >= 0])


@pytest.mark.parametrize("R", [128, 64])
@pytest.mark.parametrize("ksize", KSIZES)
def test_record_boundary_at_run_edges(pkg, coracle, field, ksize, R):
    """a record boundary at the same offsets: between two long records, and with one record of filler length (16 bases,
    valid DNA, adds nothing) wedged in between them"""
    W = ksize // 3
    for runs in run_starts(R):
        for off in edge_offsets(W, R):
            field.check(pkg, coracle, ksize, R, cuts=[p + off for p in runs])
            field.check(pkg, coracle, ksize, R, cuts=[p + off + d for p in runs if p + off > 0 for d in (0, pr.FILLER)])


@pytest.mark.parametrize("R", [128, 64])
@pytest.mark.parametrize("ksize", KSIZES)
def test_field_ends_inside_the_last_run(pkg, coracle, field, cu, ksize, R):
    """the field ends at p0 + j inside the last run, among island bases (the bases that follow in memory are valid DNA that
    must not be read as part of the batch): j below 3W (no window starts in the last run), around 3W, and j = R - 1"""
    W = ksize // 3
    p0 = cu * 1024 * 128 + 1024 if R == 128 else cu * 1024 * 64 + 256
    assert p0 % (512 * R) == (1024 if R == 128 else 256)
    for j in sorted({1, 2, 5, 3 * W - 1, 3 * W, 3 * W + 1, R // 2, R - 2, R - 1}):
        field.check(pkg, coracle, ksize, R, length=p0 + j)


@pytest.mark.parametrize("shift,ksize", [(1, 21), (3, 27), (8, 30), (15, 27)])
def test_shifted_base_pointer(pkg, coracle, cu, shift, ksize):
    """the first base 1, 3, 8 and 15 bytes past a 16-byte boundary (m, sh and xu of the staging are not zero), each with
    edge edits of both kinds, so that the shift and the edge meet"""
    f = Field(cu, shift=shift)
    W = ksize // 3
    f.check(pkg, coracle, ksize)
    for runs in run_starts(128):
        for off in edge_offsets(W, 128)[1::2]:
            f.check(pkg, coracle, ksize, edits=[(p + off, ord("N")) for p in runs])
            f.check(pkg, coracle, ksize, cuts=[p + off for p in runs])
    f.check(pkg, coracle, ksize, 64)
    f.check(pkg, coracle, ksize, 64, edits=[(p + 3 * W - 1, ord("N")) for p in run_starts(64)[1]], cuts=[p + 64 for p in run_starts(64)[1]])


@pytest.mark.parametrize("ksize", KSIZES)
def test_positions_at_runs_of_128(pkg, coracle, field, ksize):
    """k_protein_positions at R = 128: a tracked bottom-num sketch larger than the number of windows (every window is
    compared, the candidates carry positions), unedited and with edits and boundaries at the run edges"""
    W = ksize // 3
    num = 4 * MEASURED[(128, ksize)]
    field.check(pkg, coracle, ksize, mode="num", num=num)
    for runs in run_starts(128):
        for off in edge_offsets(W, 128)[::2]:
            field.check(pkg, coracle, ksize, mode="num", num=num, edits=[(p + off, ord("N")) for p in runs if p + off >= 0],
                        cuts=[p + off + 40 for p in runs])


# sketch sizes at which, for the input of the test below, the oracle's result changes both when the records are fed last to
# first and when every record is fed reverse-complemented (found by scanning num = 20 ... 1500 with the oracle on the CPU:
# 33 / 64 / 9 such sizes at ksize 21 / 27 / 30)
ORDER_NUMS = {21: (244, 510, 886, 1229), 27: (90, 301, 632, 1064), 30: (1290, 1342, 1445)}


@pytest.mark.parametrize("ksize", KSIZES)
def test_positions_decide_a_small_tracked_sketch(pkg, coracle, field, ksize):
    """num small, and the last island rewritten as a copy of the first (it holds it nearly twice, shifted by one frame).  In a full tracked bottom-num sketch the abundance of the largest hash counts only its occurrences up to the
    last first occurrence of a kept hash (quirk Q3), so with repeats late in the stream the state depends on the order the
    windows arrive in -- the six-frame order k_protein_positions has to reproduce.  That it does for these inputs is shown
    with the oracle alone: fed the records last to first, or each record reverse-complemented (the same windows, the frames
    in another order), it ends in another state."""
    first = bytes(field.base[0])
    edits = []
    for s, e in field.islands[6:]:
        edits += [(s + i, b) for i, b in enumerate((first * 3)[:e - s])]
    isl = {s: bytearray(d) for s, d in field.base.items()}
    for p, b in edits:
        s0 = max(s for s in isl if s <= p)
        isl[s0][p - s0] = b
    recs = [r for _, r in pr.island_records(isl, [], field.n128)]
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    total = sum(2 * (len(r) - 2) for r in recs)
    for num in ORDER_NUMS[ksize]:
        # the one-pass launch keeps hashes up to (2 num + 64) / positions of the hash space and is final when it shows at
        # least num distinct hashes (ingest(), bottom-num): it does here, so the fused kernel's positions are what decides
        est = int((2 * num + 64) / total * 2.0 ** 64)
        sc = coracle.MinHash(0, ksize, True, 42, est, False)
        for r in recs:
            sc.add_sequence(r, True)
        assert len(sc.mins) >= num + 50
        o = field.check(pkg, coracle, ksize, mode="small_num", num=num, edits=edits)
        assert len(o.mins) == num                               # the floor of this test: the sketch is full
        for other in (list(reversed(recs)), [r[::-1].translate(comp) for r in recs]):
            w = coracle.MinHash(num, ksize, True, 42, 0, True)
            for r in other:
                w.add_sequence(r, True)
            assert w.mins == o.mins and w.abunds != o.abunds


@pytest.mark.parametrize("ksize", KSIZES)
def test_grouped_positions_at_runs_of_128(pkg, coracle, field, ksize):
    """add_sequences_grouped_dev, the island records alternating between two scaled sketches: the fused launch hands its
    positions, rewritten by k_protein_positions, to launch_pos_to_group.  Unedited, and with boundaries at run edges
    (more island records, so the alternation falls differently)"""
    W = ksize // 3
    field.check(pkg, coracle, ksize, mode="grouped")
    for runs in run_starts(128):
        for off in (0, 3 * W - 1, 128, 128 + 3 * W):
            field.check(pkg, coracle, ksize, mode="grouped", cuts=[p + off for p in runs],
                        edits=[(p + off + 50, ord("N")) for p in runs])


R32_N = 3 * 512 * 32 + 77
R32_ISLANDS = [(0, 512), (1920, 2240), (16256, 16640), (2 * 16384 - 64, 2 * 16384 + 600)]


@pytest.mark.parametrize("ksize", KSIZES)
def test_runs_of_32(pkg, coracle, ksize):
    """R = 32 needs no device field: three 16384-base tiles and 77 bases from the host, cut like a field (the oracle's
    add_hash is quadratic in a sketch that keeps every window, so most of the input is filler here too); the same edge
    offsets, and the input ending inside the last run"""
    R, W = 32, ksize // 3
    rng = random.Random(32)
    base = pr.rand_dna(rng, R32_N)
    isl0 = {s: pr.rand_dna(rng, e - s, lower=0.3) for s, e in R32_ISLANDS}
    off0 = pr.field_offsets(R32_N, R32_ISLANDS)

    def check(edits=(), cuts=(), n=R32_N):
        isl = {s: bytearray(d) for s, d in isl0.items()}
        for p, b in edits:
            s0 = max(s for s in isl if s <= p)
            isl[s0][p - s0] = b
        seq = bytearray(base)
        for s, d in isl.items():
            seq[s:s + len(d)] = d
        cuts = [c for c in cuts if 0 < c < n]
        off = pr.with_cuts(pr.prefix_offsets(off0, n), cuts)
        case = (0, ksize, True, 42, MAXH, True)
        g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
        c = pr.route_counters(pkg, lambda: g.add_sequences([bytes(seq[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])], True))
        for _, r in pr.island_records(isl, cuts, n):
            o.add_sequence(r, True)
        assert len(o.mins) >= MEASURED[(32, ksize)] // 2
        pr.same_state(g, o)
        assert c["protein_fused"] >= 1 and c["translate"] == 0 and c["hash_windows"] == 0, c

    check()
    for runs in run_starts(R):
        for off in edge_offsets(W, R):
            check(edits=[(p + off, ord("N")) for p in runs if p + off >= 0])
            check(cuts=[p + off for p in runs])
            check(cuts=[p + off + d for p in runs if p + off > 0 for d in (0, pr.FILLER)])
    p0 = 2 * 16384 + 8 * R
    for j in sorted({1, 3 * W - 1, 3 * W, 3 * W + 1, R - 1}):
        check(n=p0 + j)
