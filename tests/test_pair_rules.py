"""The numpy model of one compared pair (pair_restatement.py) against the C oracle, on the input structures the GPU tests of
the small compare routes use and on seeded random sketches.  No GPU: test_gpu_compare_small_routes.py leans on these
functions."""
import math

import numpy as np
import pytest

import pair_restatement as PR

U64 = np.uint64


def _omh(coracle, mins, num):
    o = coracle.MinHash(num, 21, False, 42, 0)
    for h in mins.tolist():
        o.mins_push(h)            # raw push: the length does not depend on num
    return o


def _same_as_oracle(coracle, a, b, n):
    oa, ob = _omh(coracle, a, n), _omh(coracle, b, 77)      # (H6: only the num of the sketch the call is made on counts)
    common, size, cc, jac, cont = PR.pair(a, b, n)
    assert (common, size) == oa.intersection_size(ob), (n, a.size, b.size)
    assert cc == oa.count_common(ob)
    assert jac == oa.compare(ob)
    if a.size:
        assert cont == oa.containment(ob)
    else:
        assert math.isnan(cont) and math.isnan(oa.containment(ob))


def _cuts(a, b, shares):
    """0 and the nums around the end of the union, around `shares` merged elements and around the union rank reached there"""
    tot_u = PR.pair(a, b, 0)[1]
    ns = {0, 1, tot_u - 1, tot_u, tot_u + 1}
    for m in shares:
        r = PR.union_rank_of_merged_prefix(a, b, m)
        ns.update([m - 1, m, m + 1, r - 1, r, r + 1])
    return sorted(n for n in ns if n >= 0)


@pytest.mark.parametrize("total", [0, 1, 2, 7, 8, 9, 64, 129, 384, 1025])
def test_pair_is_the_oracles_pair_on_every_structure(total, coracle):
    rng = np.random.default_rng(31 + total)
    d = -(-total // 64)
    for name, a, b in PR.structures(total, rng):
        for n in _cuts(a, b, [d, 2 * d, 63 * d]):
            _same_as_oracle(coracle, a, b, n)
            _same_as_oracle(coracle, b, a, n)


def test_structures_hold_what_they_promise():
    rng = np.random.default_rng(32)
    for total in (0, 1, 3, 8, 9, 257, 768):
        got = {name: (a, b) for name, a, b in PR.structures(total, rng)}
        assert len(got) == 12
        la, lb = total // 2, total - total // 2
        for name, (a, b) in got.items():
            assert a.dtype == U64 and b.dtype == U64
            if name == "a-empty":
                assert (a.size, b.size) == (0, total)
            elif name == "b-empty":
                assert (a.size, b.size) == (total, 0)
            else:
                assert (a.size, b.size) == (la, lb), name
            both, either = np.intersect1d(a, b), np.union1d(a, b)
            if total >= 8:
                assert np.isin(PR.EXTREMES, either).all(), name
                if name.endswith("-both"):
                    assert np.isin(PR.EXTREMES, both).all(), name
                else:
                    assert not np.isin(PR.EXTREMES, both).any(), name
        if total >= 8:
            a, b = got["identical-both"]
            assert np.array_equal(a, b[np.isin(b, a)]) and np.isin(a, b).all()
            for mode in ("both", "one"):
                a, b = got["interleaved-" + mode]
                assert np.intersect1d(a, b).size == (4 if mode == "both" else 0)
                c = np.intersect1d(*got["half-overlap-" + mode]).size
                assert la // 4 <= c <= la // 2 + 4
            a, b = got["a-below-b-one"]
            assert a[-1] < b[0] and a[-1] == U64((1 << 63) - 1) and b[0] == U64(1 << 63)
            a, b = got["b-below-a-one"]
            assert b[-1] < a[0]
            a, b = got["identical-one"]
            assert np.union1d(a, b).size == lb + 2 and not np.array_equal(a, b)        # two extremes each, the bodies equal


def test_union_rank_of_merged_prefix():
    rng = np.random.default_rng(33)
    for name, a, b in PR.structures(97, rng):
        la, lb = a.tolist(), b.tolist()
        merged, i, j = [], 0, 0
        while i < len(la) or j < len(lb):                      # ties: a first
            if j >= len(lb) or (i < len(la) and la[i] <= lb[j]):
                merged.append(la[i]); i += 1
            else:
                merged.append(lb[j]); j += 1
        for m in (0, 1, 2, 48, 49, 96, 97):
            assert PR.union_rank_of_merged_prefix(a, b, m) == len(set(merged[:m])), (name, m)


@pytest.mark.parametrize("num", [0, 1, 40, 41, 300, 5000])
def test_matrix_with_one_num_is_the_oracles_matrix(num, coracle):
    rng = np.random.default_rng(34)
    pool = np.concatenate([PR.EXTREMES, rng.integers(1, (1 << 64) - 2, size=400, dtype=U64)])
    pool = np.unique(pool)
    sizes = [0, 1, 5, 40, 41, 300, 300]
    rows = [np.sort(rng.choice(pool, sizes[i % 7], replace=False)) for i in range(16)]
    cols = [np.sort(rng.choice(pool, sizes[(3 * j + 1) % 7], replace=False)) for j in range(19)]
    rows[3] = cols[2].copy()                                     # identical sketches
    rows[5] = PR.EXTREMES.copy()
    got = PR.matrix(rows, cols, num)
    common, size, jac = coracle.compare_matrix(rows, cols, num, 21, 0)
    assert (got["common"] == common).all() and (got["size"] == size).all() and (got["jaccard"] == jac).all()
    assert got["jaccard"][3, 2] == (1.0 if len(rows[3]) else 0.0)
    cc = np.array([[np.intersect1d(a, b).size for b in cols] for a in rows], dtype=U64)
    assert (got["count_common"] == cc).all()


def test_matrix_with_a_num_per_row_is_the_oracles_pair_by_pair(coracle):
    """quirk H6: row i's num truncates pair (i, j), whatever the column's num"""
    rng = np.random.default_rng(35)
    pool = np.unique(np.concatenate([PR.EXTREMES, rng.integers(1, (1 << 64) - 2, size=250, dtype=U64)]))
    rows = [np.sort(rng.choice(pool, k, replace=False)) for k in (0, 1, 64, 65, 128, 129, 200, 200, 4, 200)]
    cols = [np.sort(rng.choice(pool, k, replace=False)) for k in (0, 1, 63, 64, 200, 4)]
    cols.append(rows[6].copy())
    nums = [3, 0, 1, 64, 100, 250, 251, 252, 5000, 0]
    got = PR.matrix(rows, cols, nums)
    orow = [_omh(coracle, r, n) for r, n in zip(rows, nums)]
    ocol = [_omh(coracle, c, 9) for c in cols]
    for i, a in enumerate(orow):
        for j, b in enumerate(ocol):
            assert (int(got["common"][i, j]), int(got["size"][i, j])) == a.intersection_size(b), (i, j)
            assert int(got["count_common"][i, j]) == a.count_common(b)
            assert got["jaccard"][i, j] == a.compare(b)
            if len(rows[i]):
                assert got["containment"][i, j] == a.containment(b)
            else:
                assert np.isnan(got["containment"][i, j])
    assert (got["size"][6] == np.minimum(251, [np.union1d(rows[6], c).size for c in cols])).all()
