"""GPU parity of the protein arm's routes (ProteinSource in minhash.cpp), bit-exact against the C oracle on the whole
input: the fall-backs of the one-pass kernel (a full slow list; a candidate buffer that overflows and is rerun), the
two-pass path (k_translate + k_hash_windows) at the places where its fast paths begin and end, and launches over a part of
the position space.  Unless a test is about a threshold, every window's hash is compared: max_hash = 2^64 - 1 with
abundances, or a tracked bottom-num sketch larger than the number of windows.

The one-pass kernel serves ksize 21, 27 and 30 (windows of 7, 9, 10 residues) over the whole position space; a byte
>= 0x80 anywhere in the batch makes the library discard its launch and take the two-pass path.  The tests of that path
therefore add one record that holds nothing else -- b"\\xc3\\xa9", shorter than every ksize, so it adds nothing and
raises no error -- which brings the static instantiations k_hash_windows<7|9|10> into play; other window lengths take the two-pass
path by themselves (k_hash_windows<0>).

Every test asserts the route it is about (launch counters protein_fused, translate, hash_windows; the chunk_rerun event)
and a floor on the oracle's number of distinct windows: half of the figure written next to it, which was measured with
the oracle on the CPU."""
import random

import numpy as np
import pytest

import protein_restatement as pr

pytestmark = pytest.mark.gpu

MAXH = (1 << 64) - 1
UTF8_REC = b"\xc3\xa9"            # a record shorter than every ksize: it adds nothing and raises no error


def bad_rec(ksize):
    """a record that ends in b"\xff" after a multiple of three bases: frame 0 forward does not reach the byte and is added,
    frame 0 of the reverse complement starts with it -- from_utf8 fails there (error code 1), the rest is not added"""
    return bytes(pr.rand_dna(random.Random(ksize), 3 * ((ksize + 14) // 3))) + b"\xff"


def sketch_both(pkg, coracle, case, recs, floor, dev=None):
    """the records through the library (one batch; dev = (pointer, offsets): resident input) and through the oracle (one by
    one); error codes and states must agree, the oracle must hold at least `floor` hashes.  Returns the counters."""
    g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
    err = {}

    def run():
        try:
            if dev is not None:
                g.add_sequences_dev(dev[0], int(dev[1][-1]), dev[1], True)
            else:
                g.add_sequences(recs, True)
        except pkg.SourmashError as e:
            err["g"] = e.code

    c = pr.route_counters(pkg, run)
    for r in recs:
        try:
            o.add_sequence(r, True)
        except coracle.OracleError as e:
            err.setdefault("o", e.code)
    assert err.get("g") == err.get("o"), err
    assert len(o.mins_np()) >= floor
    pr.same_state(g, o)
    c["error"] = err.get("o")
    return c


def two_pass(pkg, coracle, ksize, recs, floor, extra=UTF8_REC, case=None, dev=None):
    """the records and one that holds a byte >= 0x80: the two-pass path does the work, at every ksize"""
    case = case or (0, ksize, True, 42, MAXH, True)
    c = sketch_both(pkg, coracle, case, list(recs) + ([extra] if extra else []), floor, dev)
    assert c["translate"] == 1 and c["hash_windows"] >= 1, c
    assert (c["protein_fused"] >= 1) == (ksize // 3 in (7, 9, 10)), c
    return c


# ------------------------------------------------------------------------------------------------------------------
# fall-backs of the one-pass kernel

def n_every_30(n, seed):
    rng = np.random.default_rng(seed)
    seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
    seq[29::30] = ord("N")
    return seq.tobytes()


def test_slow_list_overflow_takes_the_two_pass_path(pkg, coracle):
    """An 'N' every 30 bases at ksize 27: 27 of every 30 spans are not clean and are set aside for k_spliced_windows.  In
    2.2 MB that is 1.98 million, more than the list's 2^20 entries: the launch raises flag bit 2, is discarded and repeated
    on the two-pass path.  0.9 MB (0.81 million spans) stays on the one-pass kernel alone.  A test about that threshold:
    scaled 1/50 keeps the oracle quick; every kept hash carries its abundance."""
    case = (0, 27, True, 42, (1 << 64) // 50, True)
    c = sketch_both(pkg, coracle, case, [n_every_30(2_200_000, 3)], 39664)          # measured: 79328 distinct hashes kept
    assert c["protein_fused"] >= 1 and c["translate"] == 1 and c["hash_windows"] >= 1, c
    c = sketch_both(pkg, coracle, case, [n_every_30(900_000, 3)], 16165)            # measured: 32331
    assert c["protein_fused"] >= 1 and c["translate"] == 0 and c["hash_windows"] == 0, c


def test_candidate_overflow_is_rerun(pkg, coracle):
    """poly-A of 3 MB at ksize 21: every forward window is K * 7, every reverse one F * 7, so with max_hash = the larger of
    their two hashes all 2 * 3 * 10^6 windows pass where the uniform estimate expects 0.58 of them: the candidate buffer
    overflows, the counter counts on and the chunk is run again with the exact size.  Expected abundances: the closed
    form (tests/test_protein_field_rules.py).  A test about that threshold: max_hash is the larger hash, then the smaller
    one minus one, under which nothing passes."""
    n = 3_000_000
    hk, hf = coracle.hash_murmur(b"K" * 7, 42), coracle.hash_murmur(b"F" * 7, 42)
    cnt = pr.polya_windows_per_strand(n, 21)
    assert cnt == sum((n - f) // 3 - 7 + 1 for f in range(3))
    g = pkg.KmerMinHash(0, 21, True, 42, max(hk, hf), True)
    c = pr.route_counters(pkg, lambda: g.add_sequence(b"A" * n, True))
    assert dict(zip(g.mins, g.abunds)) == {hk: cnt, hf: cnt}
    assert c["chunk_rerun"] >= 1 and c["protein_fused"] >= 2 and c["translate"] == 0, c
    g = pkg.KmerMinHash(0, 21, True, 42, min(hk, hf) - 1, True)
    c = pr.route_counters(pkg, lambda: g.add_sequence(b"A" * n, True))
    assert g.mins == [] and g.abunds == []
    assert c["protein_fused"] >= 1 and c["translate"] == 0, c


def test_repeat_between_random_stretches(pkg, coracle):
    """a random stretch, "ac" * 300000, a random stretch: 1.2 million windows with four distinct hashes among 80 000 others,
    scaled (the one-pass kernel alone) and tracked bottom-num with num = 50: the one-pass launch keeps hashes up to
    164 / 1.28 million of the hash space, about ten distinct ones, fewer than num, so the growing-chunk loop takes over with
    launches over parts of the position space on the two-pass path"""
    rnd = bytes(coracle.synth_dna(0, 40000, 21, 0))
    seq = rnd[:20000] + b"ac" * 300000 + rnd[20000:]
    c = sketch_both(pkg, coracle, (0, 21, True, 42, 1 << 63, True), [seq], 20076)     # measured: 40152 distinct hashes
    assert c["protein_fused"] >= 1 and c["translate"] == 0, c
    c = sketch_both(pkg, coracle, (50, 21, True, 42, 0, True), [seq], 25)             # measured: 50, the sketch is full
    assert c["protein_fused"] >= 1 and c["translate"] == 1 and c["hash_windows"] >= 2, c


# ------------------------------------------------------------------------------------------------------------------
# k_translate: 12 bases per lane with a halo of 2, tiles of 3072 bases

TR_TILE = 3072
TR_SETS = [(0, 255 * 12), (12, TR_TILE)]          # lanes 0 and 255 of tile 0; lane 1 of tile 0 and lane 0 of tile 1
TR_N = 2 * TR_TILE + 500


@pytest.fixture(scope="module")
def tr_base():
    return pr.rand_dna(random.Random(12), TR_N, lower=0.3)


def cut(seq, cuts):
    offs = sorted({0, len(seq)} | {c for c in cuts if 0 < c < len(seq)})
    return [bytes(seq[a:b]) for a, b in zip(offs, offs[1:])]


# measured with the oracle: over all the inputs of the three tests that use it, the 6644 bases cut into records or with an
# 'N' per lane give at least 13052 / 13016 distinct windows at ksize 27 / 33 (at most 13230 / 13218)
TR_FLOOR = {27: 13052 // 2, 33: 13016 // 2}


@pytest.mark.parametrize("ksize", [27, 33])
def test_translate_record_boundary_in_a_lanes_run(pkg, coracle, tr_base, ksize):
    """a record boundary at each of the 16 bases a lane's packed path reads (its 12 bases and 2 either side): the path
    needs o >= 2 and o + 14 <= record length, so the lane and its neighbours change paths as the boundary moves"""
    for lanes in TR_SETS:
        for j in range(16):
            two_pass(pkg, coracle, ksize, cut(tr_base, [p - 2 + j for p in lanes]), TR_FLOOR[ksize])


@pytest.mark.parametrize("ksize", [27, 33])
def test_translate_bad_base_in_a_lanes_run(pkg, coracle, tr_base, ksize):
    """one 'N' at each of the same 16 bases: the packed path needs 16 clean codes"""
    for lanes in TR_SETS:
        for j in range(16):
            seq = bytearray(tr_base)
            for p in lanes:
                if p - 2 + j >= 0:
                    seq[p - 2 + j] = ord("N")
            two_pass(pkg, coracle, ksize, [bytes(seq)], TR_FLOOR[ksize])


@pytest.mark.parametrize("ksize", [27, 33])
def test_translate_short_and_tiny_records(pkg, coracle, ksize):
    """records of ksize - 1, ksize and ksize + 1 bases between long ones; 20 records of 30 / 36 bases inside one tile (more
    than 8 records start in it: lanes search for their record instead of walking); invalid UTF-8 in the extra record
    (error code 1, the frames before it kept)"""
    rng = random.Random(ksize)
    def rec(n): return bytes(pr.rand_dna(rng, n, lower=0.2))
    recs = [rec(1000), rec(ksize - 1), rec(700), rec(ksize), rec(801), rec(ksize + 1), rec(3000)]
    two_pass(pkg, coracle, ksize, recs, {27: 5400, 33: 5376}[ksize])              # measured: 10800 / 10752
    tiny = [rec(1000)] + [rec(ksize + 3) for _ in range(20)] + [rec(3000)]
    two_pass(pkg, coracle, ksize, tiny, {27: 4028, 33: 4016}[ksize])              # measured: 8056 / 8032
    c = two_pass(pkg, coracle, ksize, tiny, {27: 4030, 33: 4018}[ksize], extra=bad_rec(ksize))    # measured: 8061 / 8037
    assert c["error"] == 1


@pytest.mark.parametrize("shift", [1, 7, 15])
def test_translate_shifted_resident_input(pkg, coracle, tr_base, shift):
    """device-resident input whose first base lies 1, 7 and 15 bytes past a 16-byte boundary (the staging offset m)"""
    import torch
    recs = cut(tr_base, [1000, 1000 + 26, TR_TILE - 1, TR_TILE + 13]) + [UTF8_REC]
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    buf = torch.zeros(int(off[-1]) + shift + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + int(off[-1])] = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    for ksize in (27, 33):
        two_pass(pkg, coracle, ksize, recs, TR_FLOOR[ksize], extra=None, dev=(buf.data_ptr() + shift, off))


# ------------------------------------------------------------------------------------------------------------------
# k_hash_windows: 8 window starts per lane; murmur's structure changes at 8/9 and 16/17 residues; 33 is off the fast path

HW_KSIZES = [3, 21, 24, 27, 30, 48, 51, 96, 99]      # 21 and 30: the other two static instantiations
# measured with the oracle: distinct windows of one record of (ksize + 40 ... ksize + 63) bases and one of 200, the smallest
# over the 24 lengths; win = 1 has 21 distinct windows, the residues
HW_SWEEP_MEASURED = {3: 21, 21: 442, 30: 424, 24: 436, 27: 430, 48: 388, 51: 382, 96: 292, 99: 286}


@pytest.mark.parametrize("ksize", HW_KSIZES)
def test_hash_windows_segment_ends_in_a_lanes_run(pkg, coracle, ksize):
    """24 consecutive record lengths: the six segments of the record end at every offset of a lane's 8 starts that they can
    (tests/test_protein_field_rules.py: forward segments all eight, reverse-complement ones the even four), so the test
    g0 + 7 + win <= segment end flips at every start of a run; a second record follows, its segments begin there.  (The
    inputs are the 24 lengths; reclen_with_segment_end at the end only confirms that they reach what the helper says.)"""
    rng = random.Random(ksize)
    lo = ksize + 40
    ends = [set() for _ in range(6)]
    for n in range(lo, lo + 24):
        recs = [bytes(pr.rand_dna(rng, n, lower=0.2)), bytes(pr.rand_dna(rng, 200))]
        t = pr.segment_table([n, 200], ksize)
        for s in range(6):
            ends[s].add(t[s + 1] % 8)
        two_pass(pkg, coracle, ksize, recs, HW_SWEEP_MEASURED[ksize] // 2)
    assert [sorted(e) for e in ends] == [list(range(8)), [0, 2, 4, 6]] * 3
    for seg in range(6):
        for j in sorted(ends[seg]):
            assert lo <= pr.reclen_with_segment_end(seg, j, ksize, lo) < lo + 24


# measured with the oracle: distinct windows of the 700-base record below with one 'N' (the smallest over the positions)
HW_DROP_MEASURED = {3: 21, 21: 1354, 30: 1336, 24: 1348, 27: 1342, 48: 1300, 51: 1294, 96: 1204, 99: 1198}


@pytest.mark.parametrize("ksize", HW_KSIZES)
def test_hash_windows_dropped_codon_in_a_lanes_stretch(pkg, coracle, ksize):
    """a dropped codon at every residue of the stretch [g0, g0 + 8 + win) that lane 1 of the first segment loads, and on to
    the end of the last 8-byte word loaded, where it is outside every window of the run and the fast path is given up for
    nothing"""
    win = ksize // 3
    base = pr.rand_dna(random.Random(100 + ksize), 700, lower=0.2)
    g0 = 8
    nw = (8 + win - 1 + 7) >> 3
    assert g0 + 8 * nw >= g0 + 8 + win - 1 and 3 * (g0 + 8 * nw) + 3 * win < 700
    for r in range(g0, g0 + 8 * nw):
        seq = bytearray(base)
        seq[3 * r + 1] = ord("N")                           # residue r of frame 0, forward: segment 0 of the record
        two_pass(pkg, coracle, ksize, [bytes(seq)], HW_DROP_MEASURED[ksize] // 2)


# measured with the oracle: distinct windows of the four inputs below (202, 203, 3000 bases; 1500 and the bad record)
HW_SIZES_MEASURED = {3: (21, 21, 21, 21), 21: (364, 366, 5959, 2965), 30: (346, 348, 5942, 2947),
                     24: (358, 360, 5954, 2959), 27: (352, 354, 5948, 2953), 48: (310, 312, 5906, 2911),
                     51: (304, 306, 5900, 2905), 96: (214, 216, 5810, 2815), 99: (208, 210, 5804, 2809)}


@pytest.mark.parametrize("ksize", HW_KSIZES)
def test_hash_windows_sizes(pkg, coracle, ksize):
    """a residue count that is a multiple of 8 (a record of 202 bases: 400) and one that is not (203: 402); 5996 residues,
    three workgroups of 2048 window starts each, where every hash passes and overfills the stage of 1024 (a workgroup that
    makes several passes: test_hash_windows_several_passes_per_workgroup); invalid UTF-8 in the extra record (error code 1)"""
    rng = random.Random(200 + ksize)
    m = HW_SIZES_MEASURED[ksize]
    for i, n in enumerate((202, 203, 3000)):
        assert (2 * (n - 2)) % 8 == {202: 0, 203: 2, 3000: 4}[n]
        two_pass(pkg, coracle, ksize, [bytes(pr.rand_dna(rng, n, lower=0.2))], m[i] // 2)
    c = two_pass(pkg, coracle, ksize, [bytes(pr.rand_dna(rng, 1500))], m[3] // 2, extra=bad_rec(ksize))
    assert c["error"] == 1


# measured with the oracle: 1800 distinct windows (three units of 300 bases, 100 windows per frame and strand each), of
# which 220 lie under 2^64 / 8
SEVERAL_MEASURED = {MAXH: 1800, (1 << 64) // 8: 220}


@pytest.mark.parametrize("max_hash", [MAXH, (1 << 64) // 8])
def test_hash_windows_several_passes_per_workgroup(pkg, coracle, max_hash):
    """launch_hash_windows starts at most 16384 workgroups of 2048 window starts: beyond 33.6 million residue positions a
    workgroup makes a second pass, walks its segment forward from the first (`seg`), and carries a stage that is less than
    half full over from one pass to the next.  17.6 MB in three records of unequal length, each a unit of 300 bases
    repeated (few distinct hashes keep the oracle quick, their abundances show a window lost or hashed twice), and the
    record that forces the two-pass path.  With max_hash = 2^64 - 1 every pass overfills the stage of 1024; with 2^64 / 8
    a pass stages about 256 hashes, fewer than the 512 at which it is flushed."""
    rng = random.Random(17)
    lens = (5_000_000, 6_100_001, 6_500_002)
    recs = [(bytes(pr.rand_dna(rng, 300, lower=0.2)) * (n // 300 + 1))[:n] for n in lens]
    assert sum(2 * (n - 2) for n in lens) > 16384 * 2048 + 2048
    c = two_pass(pkg, coracle, 27, recs, SEVERAL_MEASURED[max_hash] // 2, case=(0, 27, True, 42, max_hash, True))
    assert c["hash_windows"] == 1, c                       # one launch over all positions


# ------------------------------------------------------------------------------------------------------------------
# launches over a part of the position space

@pytest.mark.parametrize("ksize", [21, 24, 27, 30])
def test_bottom_num_with_few_distinct_windows(pkg, coracle, ksize):
    """a unit of 300 bases repeated to 200 kB has 600 distinct windows (100 per frame and strand), fewer than num = 1000:
    the one-pass launch does not fill the sketch, and the growing-chunk loop runs launches over [lo, hi) with lo != 0
    (chunks of 65536, 524288, ... positions), which cross segment boundaries -- once with one record, once with two"""
    rng = random.Random(300 + ksize)
    unit = bytes(pr.rand_dna(rng, 300))
    one = (unit * 667)[:200_000]
    two = (bytes(pr.rand_dna(rng, 300)) * 667)[:200_003]
    case = (1000, ksize, True, 42, 0, True)
    for recs, measured in (([one], 600), ([one, two], 1000)):          # (the second fills the sketch: 1200 distinct)
        c = sketch_both(pkg, coracle, case, recs, measured // 2)
        assert c["hash_windows"] > 1 and c["translate"] == 1, c


def test_order_dependent_mode_in_chunks(pkg, coracle):
    """num = 8 and max_hash = 2^56 together (an order-dependent combination: add_hash is replayed in stream order), with
    abundance, ksize 27: 9 MB in three records are 18 million residue positions, more than one chunk of 2^24, so both
    launches cover a part of the position space and take the two-pass path; the second starts inside a segment"""
    import ctypes as C
    import torch
    n = 9_000_000
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    assert pkg.lib().smh_synth_dna_dev(C.c_void_p(buf.data_ptr()), 0, n, 31, 0, C.c_void_p(0)) == 0
    torch.cuda.synchronize()
    host = bytes(coracle.synth_dna(0, n, 31, 0))
    off = np.array([0, 3_000_001, 5_999_999, n], dtype=np.uint64)
    recs = [host[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]
    assert sum(2 * (len(r) - 2) for r in recs) > 1 << 24
    c = sketch_both(pkg, coracle, (8, 27, True, 42, 1 << 56, True), recs, 12960, dev=(buf.data_ptr(), off))   # measured: 25920
    assert c["hash_windows"] == 2 and c["translate"] == 1 and c["protein_fused"] == 0, c
