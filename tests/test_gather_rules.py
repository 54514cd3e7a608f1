"""Gather's rules (include/sourmash_amd.h, smh_index_gather) on the CPU: the plain-Python restatement on hand-written
cases whose rows are written out here, the committed 100-sketch fixture, and the C ABI's two new symbols."""
import ctypes as C

import pytest

import gather_restatement as GR

U = GR.UNASSIGNED


def row(match, remaining, original, size, abund):
    return {"match": match, "common_remaining": remaining, "common_original": original, "size_match": size, "abund_sum": abund}


def test_tie_goes_to_the_lowest_index():
    # sketches 1 and 2 both hold two query hashes: 1 wins; 2 is left with one and follows
    rows, assigned = GR.gather([[9], [1, 2, 50], [2, 3], [60]], [1, 2, 3, 9, 70])
    assert rows == [row(1, 2, 2, 3, 2), row(0, 1, 1, 1, 1), row(2, 1, 2, 2, 1)]
    assert assigned == [0, 0, 2, 1, U]
    assert GR.ties([[9], [1, 2, 50], [2, 3], [60]], [1, 2, 3, 9, 70]) == [0, 1]


def test_duplicate_sketch_is_never_reported():
    rows, assigned = GR.gather([[5, 6, 7], [1], [5, 6, 7]], [1, 5, 6, 7])
    assert rows == [row(0, 3, 3, 3, 3), row(1, 1, 1, 1, 1)]
    assert assigned == [1, 0, 0, 0]


def test_sketch_swallowed_by_an_earlier_one():
    # sketch 1 is a subset of sketch 0: nothing of it is left after round 0; abundances are summed over what a row consumed
    ab = {1: 10, 2: 20, 3: 30, 4: 40, 8: 5}
    rows, assigned = GR.gather([[1, 2, 3, 4], [2, 3], [4, 8]], [1, 2, 3, 4, 8], ab)
    assert rows == [row(0, 4, 4, 4, 100), row(2, 1, 2, 2, 5)]
    assert assigned == [0, 0, 0, 0, 1]


def test_threshold_and_its_zero():
    sk = [[1, 2, 3], [4, 5], [6]]
    q = [1, 2, 3, 4, 5, 6]
    assert [r["match"] for r in GR.gather(sk, q, threshold=0)[0]] == [0, 1, 2]      # 0 is read as 1
    assert [r["match"] for r in GR.gather(sk, q, threshold=1)[0]] == [0, 1, 2]
    rows, assigned = GR.gather(sk, q, threshold=2)
    assert rows == [row(0, 3, 3, 3, 3), row(1, 2, 2, 2, 2)] and assigned == [0, 0, 0, 1, 1, U]
    assert GR.gather(sk, q, threshold=4) == ([], [U] * 6)


def test_capacity():
    sk = [[1, 2, 3], [4, 5], [6]]
    q = [1, 2, 3, 4, 5, 6]
    assert GR.gather(sk, q, capacity=0) == ([], [U] * 6)
    rows, assigned = GR.gather(sk, q, capacity=2)
    assert [r["match"] for r in rows] == [0, 1] and assigned == [0, 0, 0, 1, 1, U]
    assert len(GR.gather(sk, q, capacity=3)[0]) == 3 and len(GR.gather(sk, q, capacity=1000)[0]) == 3
    full = GR.gather(sk, q)
    for cap in (0, 1, 2, 3, 1000):
        assert GR.cut(*full, cap) == GR.gather(sk, q, capacity=cap)


def test_zero_rows_without_error():
    assert GR.gather([], [1, 2]) == ([], [U, U])
    assert GR.gather([[1], [2]], []) == ([], [])
    assert GR.gather([[], []], [1]) == ([], [U])
    assert GR.gather([[5], [6]], [1, 2]) == ([], [U, U])


def test_derived_values_and_threshold_in_bp():
    rows, assigned = GR.gather([[1, 2, 3, 4], [2, 3], [4, 8]], [1, 2, 3, 4, 8], {1: 10, 2: 20, 3: 30, 4: 40, 8: 5})
    d = GR.derived(rows, assigned, 5, [10, 20, 30, 40, 5], 1000)
    assert d[0] == {"f_orig_query": 0.8, "f_match": 1.0, "f_unique_to_query": 0.8, "f_unique_weighted": 100 / 105,
                    "average_abund": 25.0, "remaining_bp": 1000}
    assert d[1] == {"f_orig_query": 0.4, "f_match": 0.5, "f_unique_to_query": 0.2, "f_unique_weighted": 5 / 105,
                    "average_abund": 5.0, "remaining_bp": 0}
    assert [GR.threshold_common(bp, 1000) for bp in (0, 1, 1000, 1001, 50000)] == [0, 1, 1, 2, 50]


def test_fixture_decomposition(sbt_subset_sketches):
    """the 100 sketches of the committed SBT fixture against the union of all of them"""
    sk = [s["mins"] for s in sbt_subset_sketches]
    query = sorted(set().union(*sk))
    rows, assigned = GR.gather(sk, query, threshold=1)
    assert len(rows) == 99
    assert len(GR.ties(sk, query, threshold=1)) == 7
    assert [(r["match"], r["common_remaining"]) for r in rows[:5]] == [(29, 16140), (84, 4552), (91, 4143), (40, 3541), (50, 3393)]
    assert len(GR.gather(sk, query, threshold=50)[0]) == 82
    assert sorted(set(assigned)) == list(range(99))       # the query is the union: every position is consumed
    assert sum(r["common_remaining"] for r in rows) == len(query)


def test_gather_is_exported_and_fails_loudly_without_gpu(pkg):
    L = pkg.lib()
    assert {"smh_index_gather", "smh_gather_rounds_per_sync"} <= set(pkg.exported_symbols())
    assert L.smh_gather_rounds_per_sync() >= 1
    assert hasattr(pkg.index.ResidentIndex, "gather")
    if pkg.device_available():
        return   # with a device the call itself is the business of test_gpu_gather.py
    # no resident index can exist without a device; the entry point itself says what is missing, and writes nothing
    q = pkg.KmerMinHash(0, 21, False, 42, 1 << 60)
    for h in (7, 11, 13):
        q.add_hash(h)
    rows = (pkg._lib.SmhGatherRow * 4)()
    n_rows = C.c_uint32(77)
    code = L.smh_index_gather(None, q._p, 1, rows, 4, C.byref(n_rows), None)
    assert code == 2
    with pytest.raises(pkg.SourmashError) as ei:
        pkg.errors.check()
    assert ei.value.code == 2 and "no HIP device available" in ei.value.message
    assert n_rows.value == 77 and q.mins == [7, 11, 13]
    with pytest.raises(pkg.SourmashError) as ei:
        pkg.index.ResidentIndex([q]).gather(q)
    assert ei.value.code == 2
