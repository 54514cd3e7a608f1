"""The numpy model of the fold (fold_restatement.py) against the C oracle on seeded random inputs, and the sort checker
against numpy's stable sort.  No GPU: the GPU tests of the fold, the device union and the sort lean on these functions."""
import numpy as np
import pytest

import fold_restatement as FR

U64 = np.uint64
MX = 1 << 61


def _state(o, track):
    return o.mins_np(), (o.abunds_np() if track else None)


def _same(got, o, track):
    assert np.array_equal(got[0], o.mins_np())
    if track:
        assert np.array_equal(got[1], o.abunds_np())
    else:
        assert got[1] is None and o.abunds is None


@pytest.mark.parametrize("track", [True, False])
def test_scaled_add_is_the_oracles_add_many(track, coracle):
    rng = np.random.default_rng(21)
    universe = rng.integers(0, 1 << 62, size=20_000, dtype=U64)          # about half of them <= max_hash
    universe[:4] = [0, MX, MX + 1, (1 << 64) - 1]                        # the threshold itself is a member, one above is not
    o = coracle.MinHash(0, 21, False, 42, MX, track)
    state = (np.zeros(0, dtype=U64), np.zeros(0, dtype=U64) if track else None)
    for size in (0, 1, 50_000, 7_000):                                   # into an empty sketch, then into a filled one
        stream = universe[rng.integers(0, universe.size, size=size)]
        o.add_many(stream)
        state = FR.scaled_add(state[0], state[1], stream, MX, track)
        _same(state, o, track)
    assert 5_000 < state[0].size < 15_000 and (state[0] <= U64(MX)).all()
    if track:
        assert int(state[1].max()) > 3


@pytest.mark.parametrize("num", [1, 500, 3_000])
def test_num_add_untracked_is_the_oracles_add_many(num, coracle):
    rng = np.random.default_rng(22 + num)
    universe = rng.integers(0, 1 << 64, size=20_000, dtype=U64)
    universe[:2] = [0, (1 << 64) - 1]
    o = coracle.MinHash(num, 21, False, 42, 0, False)
    mins = np.zeros(0, dtype=U64)
    for size in (num // 2, 30_000, 5_000):                                # not full yet, full, full and fed again
        stream = universe[rng.integers(0, universe.size, size=size)]
        o.add_many(stream)
        mins = FR.num_add_untracked(mins, stream, num)
        assert np.array_equal(mins, o.mins_np())
    assert mins.size == num


def test_union_parts_is_add_hash_hash_by_hash(coracle):
    """tracked: every hash of every part added abundance times through add_hash; untracked: once"""
    rng = np.random.default_rng(23)
    universe = np.unique(rng.integers(0, MX, size=6_000, dtype=U64))
    parts = []
    for size in (1_500, 0, 1, 2_500, 700):
        m = np.sort(rng.choice(universe, size=size, replace=False))
        parts.append((m, rng.integers(1, 6, size=size).astype(U64)))
    for track in (True, False):
        o = coracle.MinHash(0, 21, False, 42, MX, track)
        state = (np.zeros(0, dtype=U64), np.zeros(0, dtype=U64) if track else None)
        for upto in (2, len(parts)):                                      # a first union, then one into a non-empty state
            batch = parts[:upto] if upto == 2 else parts[2:]
            for m, a in batch:
                for h, c in zip(m.tolist(), a.tolist()):
                    for _ in range(c if track else 1):
                        o.add_hash(h)
            state = FR.union_parts(state[0], state[1], [(m, a if track else None) for m, a in batch])
            _same(state, o, track)
        assert state[0].size > 3_000


def test_union_parts_is_the_oracles_merge(coracle):
    """two tracked scaled sketches merged (reference src/lib.rs:307-403): the union, abundances summed -- including sums
    that cross 2^32, written into the oracle's vectors directly"""
    rng = np.random.default_rng(24)
    universe = np.unique(rng.integers(0, MX, size=20_000, dtype=U64))
    big = np.array([1, (1 << 32) - 1, 1 << 32, 1 << 40], dtype=U64)
    sides = []
    for size in (12_000, 11_000):
        m = np.sort(rng.choice(universe, size=size, replace=False))
        sides.append((m, big[rng.integers(0, 4, size=size)]))
    oa, ob = (coracle.MinHash(0, 21, False, 42, MX, True) for _ in range(2))
    for o, (m, a) in zip((oa, ob), sides):
        for h, c in zip(m.tolist(), a.tolist()):
            o.mins_push(h); o.abunds_push(c)
    oa.merge(ob)
    got = FR.union_parts(sides[0][0], sides[0][1], [sides[1]])
    _same(got, oa, True)
    common = np.intersect1d(sides[0][0], sides[1][0]).size
    assert common > 3_000 and got[0].size == 23_000 - common
    assert int(got[1].max()) == 1 << 41 and ((got[1] > U64(1 << 32)) & (got[1] < U64(1 << 33))).any()


def test_sort_checker_agrees_with_numpys_stable_sort():
    rng = np.random.default_rng(25)
    for keys in (rng.integers(0, 1 << 64, size=5_000, dtype=U64), rng.integers(0, 40, size=5_000, dtype=U64),
                 np.full(300, 7, dtype=U64), np.zeros(0, dtype=U64), np.array([3], dtype=U64)):
        order = np.argsort(keys, kind="stable").astype(np.uint32)
        assert FR.check_sorted_with_payload(keys, keys[order], order) is None


def test_sort_checker_rejects_what_a_wrong_sort_returns():
    rng = np.random.default_rng(26)
    keys = rng.integers(0, 40, size=5_000, dtype=U64)                     # about 125 copies of every key
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    out = keys[order]
    t = int(np.flatnonzero(out[1:] == out[:-1])[17])                      # two neighbours with the same key
    swapped = order.copy()
    swapped[[t, t + 1]] = swapped[[t + 1, t]]
    assert FR.check_sorted_with_payload(keys, out, swapped) == "equal keys changed their order"
    d = int(np.flatnonzero(out[1:] != out[:-1])[5])                       # two neighbours with different keys
    bad = order.copy()
    bad[[d, d + 1]] = bad[[d + 1, d]]
    assert FR.check_sorted_with_payload(keys, out, bad) == "a key does not sit with its payload"
    bad_keys = out.copy()
    bad_keys[[d, d + 1]] = bad_keys[[d + 1, d]]
    assert FR.check_sorted_with_payload(keys, bad_keys, bad) == "keys_out descends somewhere"
    twice = order.copy()
    twice[t + 1] = twice[t]
    assert FR.check_sorted_with_payload(keys, out, twice) == "payload is not a permutation"
    far = order.copy()
    far[0] = keys.size
    assert FR.check_sorted_with_payload(keys, out, far) == "payload out of range"
    assert FR.check_sorted_with_payload(keys, out[:-1], order[:-1]) == "sizes differ"
