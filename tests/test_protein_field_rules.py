"""CPU checks of the claims that tests/test_gpu_protein_fused_edges.py and tests/test_gpu_protein_routes.py lean on, with
the oracles only (no product code): the field rule, the closed-form window count of poly-A, and the record-length helper
of the segment-end sweep against the six-frame layout of ProteinSource::ensure_segments restated in
tests/protein_restatement.py."""
import random

import numpy as np
import pytest

import protein_restatement as pr

MAXH = (1 << 64) - 1


def _state(o):
    return o.mins, o.abunds


def _reduced_field(seed):
    """3000 filler records of 16 valid bases around three islands of mixed-case DNA; returns (bytes, offsets, islands)"""
    rng = random.Random(seed)
    islands = [(0, 400), (16000, 16000 + 333), (40000 - 500, 40000 + 77)]
    n = 40000 + 77
    field = pr.rand_dna(rng, n)
    isl = {}
    for s, e in islands:
        isl[s] = bytes(pr.rand_dna(rng, e - s, lower=0.3))
        field[s:e] = isl[s]
    return bytes(field), pr.field_offsets(n, islands), isl, n


@pytest.mark.parametrize("ksize", [21, 27, 30])
def test_filler_records_add_nothing(ksize, coracle, pyoracle):
    """records shorter than ksize add nothing in the protein arm (src/lib.rs:257): the field fed whole, record by record,
    leaves the state that the island records alone leave -- scaled with every hash kept, and bottom-num with abundance"""
    field, off, isl, n = _reduced_field(5)
    lens = np.diff(off.astype(np.int64))
    assert len(lens) > 2000 and int((lens == pr.FILLER).sum()) > 2000 and int((lens >= ksize).sum()) == 3
    recs = pr.island_records(isl, [], n)
    assert [len(r) for _, r in recs] == [400, 333, 577]
    for case in [(0, ksize, True, 42, MAXH, True), (5000, ksize, True, 42, 0, True), (50, ksize, True, 42, 0, True)]:
        a, b = coracle.MinHash(*case), coracle.MinHash(*case)
        for x, y in zip(off[:-1], off[1:]):
            a.add_sequence(field[int(x):int(y)], True)
        for _, r in recs:
            b.add_sequence(r, True)
        assert _state(a) == _state(b)
        # measured with the oracle: 2500 / 2464 / 2446 distinct windows at ksize 21 / 27 / 30 (all windows are distinct)
        if case[0] != 50:
            assert len(b.mins) >= {21: 1250, 27: 1232, 30: 1223}[ksize]
            assert sum(b.abunds) == sum(pr.window_count(len(r), ksize) for _, r in recs)
    # the Python oracle agrees on the rule (one island and its neighbours)
    p, q = pyoracle.MinHash(0, ksize, True, 42, MAXH, True), pyoracle.MinHash(0, ksize, True, 42, MAXH, True)
    for x, y in zip(off[:40], off[1:41]):
        p.add_sequence(field[int(x):int(y)], True)
    q.add_sequence(recs[0][1], True)
    assert list(p.mins) == list(q.mins) and list(p.abunds) == list(q.abunds) and len(q.mins) > 300


def test_field_offsets_layout():
    """the field cutter: islands are whole records, everything else is shorter than every ksize under test"""
    islands = [(0, 1024), (3840, 4480), (8000, 8100)]
    for n in (8100, 8099, 8050, 9001, 4000):
        off = pr.field_offsets(n, islands)
        assert off[0] == 0 and off[-1] == n
        lens = np.diff(off.astype(np.int64))
        long_ = [(int(a), int(b)) for a, b in zip(off[:-1], off[1:]) if b - a > pr.FILLER]
        assert long_ == [(s, min(e, n)) for s, e in islands if min(e, n) - s > pr.FILLER]
        assert lens.min() >= 1 and (lens <= pr.FILLER).sum() == len(lens) - len(long_)
    off = pr.with_cuts(pr.field_offsets(8100, islands), [100, 116, 4000])
    assert {100, 116, 4000} <= set(off.tolist()) and (np.diff(off.astype(np.int64)) > 0).all()
    recs = pr.island_records({0: b"a" * 1024, 3840: b"c" * 640}, [100, 116, 4000, 7000], 4100)
    assert [(s, len(r)) for s, r in recs] == [(0, 100), (100, 16), (116, 908), (3840, 160), (4000, 100)]


@pytest.mark.parametrize("n", [21, 22, 23, 100, 3_000_000])
def test_polya_closed_form(n, coracle):
    """poly-A through the protein arm at ksize 21: the forward windows are all K * 7, the reverse ones all F * 7, and there
    are (n - f) // 3 - 7 + 1 of each per frame f"""
    o = coracle.MinHash(0, 21, True, 42, MAXH, True)
    o.add_sequence(b"A" * n, True)
    hk, hf = coracle.hash_murmur(b"K" * 7, 42), coracle.hash_murmur(b"F" * 7, 42)
    cnt = pr.polya_windows_per_strand(n, 21)
    assert cnt == sum((n - f) // 3 - 7 + 1 for f in range(3)) and 2 * cnt == pr.window_count(n, 21)
    assert dict(zip(o.mins, o.abunds)) == {hk: cnt, hf: cnt}


@pytest.mark.parametrize("ksize", [3, 24, 27, 48, 51, 96, 99])
def test_record_length_for_a_segment_end(ksize, coracle):
    """reclen_with_segment_end against the restated layout: over 24 consecutive record lengths the forward segments end at
    every offset 0..7 of a run of 8 window starts, the reverse-complement ones (an even number of residues before their
    end) at every even offset; and the layout's total is the number of residues the oracle makes windows of"""
    lo = ksize + 40
    for base_rec in (None, 1000, 1003):                 # the record alone, and after one of 1996 / 2002 residues
        lens0 = [] if base_rec is None else [base_rec]
        base = pr.segment_table(lens0, ksize)[-1]
        for seg in range(6):
            reached = set()
            for j in range(8):
                n = pr.reclen_with_segment_end(seg, j, ksize, lo, base)
                if n is None:
                    continue
                assert lo <= n < lo + 24
                t = pr.segment_table(lens0 + [n], ksize)
                assert t[6 * len(lens0) + seg + 1] % 8 == j
                reached.add(j)
            assert reached == (set(range(8)) if seg % 2 == 0 else {0, 2, 4, 6})
    # the layout's segment lengths are what the oracle windows: one clean record, every window counted
    rng = random.Random(ksize)
    for n in (ksize - 1, ksize, ksize + 1, lo, lo + 7):
        o = coracle.MinHash(0, ksize, True, 42, MAXH, True)
        o.add_sequence(bytes(pr.rand_dna(rng, n)), True)
        w = ksize // 3
        assert sum(o.abunds) == sum(max(0, s - w + 1) for s in pr.segment_lengths(n, ksize)) == pr.window_count(n, ksize)
