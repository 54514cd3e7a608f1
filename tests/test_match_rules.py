"""The rules of matching records (include/sourmash_amd.h, "Matching records") as tests/match_restatement.py restates them,
pinned on cases small enough to check by hand.  No GPU, no product import: tests/test_gpu_match.py holds the library to this."""
import pytest

import match_restatement as R

SEQ30 = b"CTCGAATAAAAGTAGACTTCACGCCCTTAA"   # pyoracle.synth_dna(0, 30, 11)
# murmur64 (seed 42) of the canonical 21-mers of SEQ30, in window order: pyoracle.hash_murmur(min(kmer, revcomp(kmer)))
HASHES30 = [7941577506958342359, 7052271885388151487, 2411703374284256564, 13988949086558266027, 7537081340606148443,
            3628592310221851221, 3265389935186436716, 17664656394686760855, 12396656035890660969, 8406165417579525362]
KMER = b"ACGTTGCAAGGCTTACCGATA"


def test_the_ten_windows_of_a_thirty_base_record(pyoracle):
    assert pyoracle.synth_dna(0, 30, 11) == SEQ30
    assert R.window_hashes(SEQ30, 21) == HASHES30
    for p in range(10):
        kmer = SEQ30[p:p + 21]
        assert pyoracle.hash_murmur(min(kmer, pyoracle.revcomp(kmer)), 42) == HASHES30[p]
    rows, off, flat = R.match([SEQ30], 21, 42, R.U64_MAX, [[HASHES30[2], HASHES30[7], 5], [HASHES30[7]]])
    assert rows == [(10, 10, 2, 2, 0, 2)]
    assert off == [0, 2] and flat == sorted([HASHES30[2], HASHES30[7]])
    # shorter than k, exactly k, k + 1
    rows, _, _ = R.match([SEQ30[:20], SEQ30[:21], SEQ30[:22], b""], 21, 42, R.U64_MAX, [[HASHES30[0]]])
    assert rows == [(0, 0, 0, 0, R.MISS, 0), (1, 1, 1, 1, 0, 1), (2, 2, 1, 1, 0, 1), (0, 0, 0, 0, R.MISS, 0)]


def test_a_kmer_and_its_reverse_complement_are_one_hash(pyoracle):
    rc = pyoracle.revcomp(KMER)
    assert rc == b"TATCGGTAAGCCTTGCAACGT" and R.kmer_hash(KMER) == R.kmer_hash(rc) == 4349023022119915064
    rec = KMER + rc                      # its own reverse complement: window p and window 21 - p are one k-mer
    hs = R.window_hashes(rec, 21)
    assert len(hs) == 22 and hs[0] == hs[21] and all(hs[p] == hs[21 - p] for p in range(22))
    rows, off, flat = R.match([rec], 21, 42, R.U64_MAX, [[hs[0]]])
    assert rows == [(22, 11, 2, 1, 0, 1)] and flat == [hs[0]] and off == [0, 1]
    assert R.window_hashes(rec.lower(), 21) == hs


def test_an_n_knocks_out_exactly_k_windows(pyoracle):
    seq = bytearray(pyoracle.synth_dna(100, 60, 5))
    whole = R.window_hashes(bytes(seq), 21)
    assert len(whole) == 40
    seq[30] = ord("N")
    left = R.window_hashes(bytes(seq), 21)
    assert len(left) == 40 - 21 and left == whole[:10] + whole[31:]
    seq[0] = seq[59] = ord("N")          # the first and the last byte: one window each
    assert R.window_hashes(bytes(seq), 21) == whole[1:10] + whole[31:39]
    assert R.window_hashes(b"ACGTN" * 12, 21) == []   # an N in every window


def test_the_tie_goes_to_the_lowest_node_and_no_hit_has_no_best():
    a, b, c = HASHES30[1], HASHES30[4], HASHES30[8]
    nodes = [[1], [2], [b, c], [], [], [a, b], [3]]
    rows, _, _ = R.match([SEQ30], 21, 42, R.U64_MAX, nodes)
    assert rows == [(10, 10, 3, 3, 2, 2)]          # nodes 2 and 5 hold two each
    rows, _, _ = R.match([SEQ30], 21, 42, R.U64_MAX, list(reversed(nodes)))
    assert rows[0][4:] == (1, 2)
    rows, off, flat = R.match([SEQ30], 21, 42, R.U64_MAX, [[1, 2, 3], []])
    assert rows == [(10, 10, 0, 0, R.MISS, 0)] and off == [0, 0] and flat == []
    # three nodes, identical: the first
    assert R.match([SEQ30], 21, 42, R.U64_MAX, [[a, c]] * 3)[0] == [(10, 10, 2, 2, 0, 2)]


def test_the_compare_with_max_hash_is_inclusive_and_unsigned():
    lo = min(HASHES30)
    assert lo == 2411703374284256564
    assert R.match([SEQ30], 21, 42, lo, [[lo]])[0] == [(1, 1, 1, 1, 0, 1)]
    assert R.match([SEQ30], 21, 42, lo - 1, [[lo]])[0] == [(0, 0, 0, 0, R.MISS, 0)]
    big = [h for h in HASHES30 if h >= 1 << 63]     # hashes a signed compare would put below zero
    assert len(big) == 3
    assert R.match([SEQ30], 21, 42, (1 << 63) - 1, [HASHES30])[0] == [(7, 7, 7, 7, 0, 7)]


def test_a_window_never_spans_two_records():
    rows, off, flat = R.match([SEQ30[:15], SEQ30[15:]], 21, 42, R.U64_MAX, [HASHES30])
    assert rows == [(0, 0, 0, 0, R.MISS, 0)] * 2 and off == [0, 0, 0]
    rows, off, flat = R.match([SEQ30[:25], SEQ30[5:]], 21, 42, R.U64_MAX, [HASHES30])
    assert rows == [(5, 5, 5, 5, 0, 5)] * 2 and off == [0, 5, 10] and flat == sorted(HASHES30[:5]) + sorted(HASHES30[5:])


def test_the_index_that_is_refused():
    ok = ("DNA", 0, 21, 42, 1 << 60)
    assert R.check_index([ok, ok]) == (21, 42, 1 << 60)
    for bad in (("protein", 0, 21, 42, 1 << 60), ("DNA", 500, 21, 42, 0), ("DNA", 0, 21, 42, 1 << 59), ("DNA", 0, 31, 42, 1 << 60),
                ("DNA", 0, 21, 43, 1 << 60)):
        with pytest.raises(R.Refused):
            R.check_index([ok, bad])
    with pytest.raises(R.Refused):
        R.check_index([])
