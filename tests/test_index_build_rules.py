"""The rules of building an index from records and of concatenation (include/sourmash_amd.h, "Building an index from
records") on the plain-Python restatement alone: hand-written cases against literal sets, and each refusal's condition.
No device."""
import pytest

import index_build_restatement as IB
import match_restatement as MR

K = 5
DNA = dict(num=0, ksize=K, molecule="DNA", seed=42, max_hash=IB.U64_MAX, track=True)
FLAT = dict(DNA, track=False)


def H(kmer):
    return MR.kmer_hash(kmer)


def split(off, xs):
    return [xs[off[g]:off[g + 1]] for g in range(len(off) - 1)]


def test_interleaved_group_ids_feed_their_own_nodes():
    recs = [b"ACGTA", b"CCCCC", b"GATTA", b"TTGCA"]
    off, h, ab = IB.build(recs, [1, 0, 1, 0], 2, DNA)
    assert split(off, h) == [sorted({H(b"CCCCC"), H(b"TTGCA")}), sorted({H(b"ACGTA"), H(b"GATTA")})]
    assert ab == [1, 1, 1, 1] and off == [0, 2, 4]


@pytest.mark.parametrize("groups,want_sizes", [([2, 2], [0, 0, 1]), ([0, 2], [1, 0, 1]), ([0, 0], [1, 0, 0])])
def test_empty_groups_first_middle_and_last_are_empty_nodes(groups, want_sizes):
    off, h, _ = IB.build([b"ACGTA", b"ACGTA"], groups, 3, DNA)
    assert [off[g + 1] - off[g] for g in range(3)] == want_sizes
    assert set(h) == {H(b"ACGTA")}


def test_no_groups_means_one_node_per_record_and_zero_groups_an_empty_index():
    off, h, _ = IB.build([b"ACGTA", b"GATTA"], None, 2, DNA)
    assert split(off, h) == [[H(b"ACGTA")], [H(b"GATTA")]]
    assert IB.build([], None, 0, DNA) == ([0], [], [])
    assert IB.build([], [], 0, FLAT) == ([0], [], None)


def test_records_shorter_than_k_add_nothing():
    off, h, ab = IB.build([b"ACGT", b"", b"ACGTAC"], [0, 0, 1], 2, DNA)
    assert off[1] == 0 and split(off, h)[1] == sorted({H(b"ACGTA"), H(b"CGTAC")})


def test_a_window_holding_n_is_skipped_and_the_others_kept():
    # windows: ACGTA, CGTAN, GTANC, TANCC, ANCCG, NCCGG, CCGGA -- five hold the N
    off, h, ab = IB.build([b"ACGTANCCGGA"], None, 1, DNA)
    assert h == sorted({H(b"ACGTA"), H(b"CCGGA")}) and ab == [1, 1]


def test_lower_case_and_reverse_complement_are_one_hash():
    assert H(b"acgta") == H(b"ACGTA") == H(b"TACGT")
    off, h, ab = IB.build([b"acgta", b"TACGT"], [0, 0], 1, DNA)
    assert h == [H(b"ACGTA")] and ab == [2]


def test_counts_are_added_across_the_records_of_a_group_only():
    recs = [b"AAAAAAA", b"AAAAA", b"AAAAAA"]     # 3, 1 and 2 windows of AAAAA
    off, h, ab = IB.build(recs, [0, 1, 0], 2, DNA)
    assert h == [H(b"AAAAA"), H(b"AAAAA")] and ab == [5, 1]
    assert IB.build(recs, [0, 1, 0], 2, FLAT)[2] is None


def test_sampling_keeps_hashes_up_to_max_hash_inclusive():
    hs = sorted({H(b"ACGTA"), H(b"GATTA"), H(b"CCCCC")})
    off, h, _ = IB.build([b"ACGTA", b"GATTA", b"CCCCC"], [0, 0, 0], 1, dict(DNA, max_hash=hs[1]))
    assert h == hs[:2]


def test_hashes_ascend_as_unsigned_across_2_63():
    lo, hi = (1 << 63) - 1, 1 << 63
    off, h, ab = IB.csr([{hi: 2, lo: 1, IB.U64_MAX: 3, 0: 4}], True)
    assert h == [0, lo, hi, IB.U64_MAX] and ab == [4, 1, 2, 3]


def test_2_32_minus_1_is_kept_and_2_32_refused_naming_the_lowest_group():
    keep = (1 << 32) - 1
    assert IB.csr([{7: keep}], True)[2] == [keep]
    with pytest.raises(IB.Refused, match="group 1 "):
        IB.csr([{7: keep}, {7: 1 << 32}, {8: 1 << 33}], True)
    assert IB.csr([{7: 1 << 32}], False) == ([0, 1], [7], None)   # nothing is counted without abundances


def test_amino_input_and_the_translated_arm_follow_the_oracle_sketches():
    import amino_restatement as AR
    prot = dict(num=0, ksize=9, molecule="protein", seed=42, max_hash=IB.U64_MAX, track=True)
    off, h, ab = IB.build([b"MKVLAA", b"MKV"], [0, 0], 1, prot, IB.AMINO)
    want = AR.amino_sketch([b"MKVLAA", b"MKV"], "protein", 9, 0, IB.U64_MAX, True)
    assert h == want.mins and ab == want.abunds and ab[h.index(want.mins[0])] >= 1
    dna = b"ATGAAAGTTCTGGCAGCA"
    off, h, ab = IB.build([dna], None, 1, dict(prot, molecule="dayhoff"))
    want = AR.translated_sketch([dna], "dayhoff", 9, 0, IB.U64_MAX, True)
    assert h == want.mins and ab == want.abunds and len(h) > 0


def test_every_refusal_has_its_condition():
    recs, groups = [b"ACGTA", b"GATTA"], [0, 1]
    IB.check(DNA, IB.NUCLEOTIDE, recs, groups, 2)
    with pytest.raises(IB.Refused, match="like is NULL"):
        IB.check(None, IB.NUCLEOTIDE, recs, groups, 2)
    with pytest.raises(IB.Refused, match="NULL"):
        IB.check(DNA, IB.NUCLEOTIDE, None, groups, 2)
    with pytest.raises(IB.Refused, match="unknown input"):
        IB.check(DNA, 2, recs, groups, 2)
    with pytest.raises(IB.Refused, match="not a scaled"):
        IB.check(dict(DNA, num=500, max_hash=0), IB.NUCLEOTIDE, recs, groups, 2)
    with pytest.raises(IB.Refused, match="not a scaled"):
        IB.check(dict(DNA, num=0, max_hash=0), IB.NUCLEOTIDE, recs, groups, 2)
    with pytest.raises(IB.Refused, match="amino-acid input"):
        IB.check(DNA, IB.AMINO, recs, groups, 2)
    with pytest.raises(IB.Refused, match=r"ascend \(record 1\)"):
        IB.check(DNA, IB.NUCLEOTIDE, recs, groups, 2, offsets=[0, 5, 4])
    with pytest.raises(IB.Refused, match="beyond"):
        IB.check(DNA, IB.NUCLEOTIDE, recs, groups, 2, offsets=[0, 5, 10], total_len=9)
    IB.check(DNA, IB.NUCLEOTIDE, recs, groups, 2, offsets=[0, 5, 10], total_len=10)
    with pytest.raises(IB.Refused, match=r"groups\[1\] is 2"):
        IB.check(DNA, IB.NUCLEOTIDE, recs, [0, 2], 2)
    with pytest.raises(IB.Refused, match="groups is NULL"):
        IB.check(DNA, IB.NUCLEOTIDE, recs, None, 3)
    with pytest.raises(IB.Refused, match="window size"):
        IB.check(dict(DNA, ksize=0), IB.NUCLEOTIDE, recs, groups, 2)
    with pytest.raises(IB.Refused, match="window size"):
        IB.check(dict(DNA, ksize=2, molecule="hp"), IB.AMINO, recs, groups, 2)
    with pytest.raises(IB.Refused, match="2\\^24"):
        IB.check(DNA, IB.NUCLEOTIDE, recs, groups, 1 << 24)
    IB.check(DNA, IB.NUCLEOTIDE, recs, groups, (1 << 24) - 1)


def test_concat_joins_nodes_in_order_and_rebases_offsets():
    a = ([0, 2, 2], [5, 9], [1, 2])
    b = ([3, 4], [7], [3])                       # a part whose offsets do not start at 0
    assert IB.concat([a, b]) == ([0, 2, 2, 3], [5, 9, 7], [1, 2, 3])
    assert IB.concat([]) == ([0], [], [])
    assert IB.concat([a]) == a
    assert IB.concat([([0], [], []), a, ([0], [], [])]) == a
    flat = ([0, 1], [4], None)
    assert IB.concat([a, flat]) == ([0, 2, 2, 3], [5, 9, 4], None)
    with pytest.raises(IB.Refused, match=r"parts\[1\] is NULL"):
        IB.concat([a, None])
    with pytest.raises(IB.Refused, match="parts is NULL"):
        IB.concat(None)
