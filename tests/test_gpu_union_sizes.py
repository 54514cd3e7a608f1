"""The union of a sketch resident in HBM with sorted distinct parts (sort.hip sorted_union_async and its host driver), driven
with plain integer arrays through absorb_dev and read back through export_dev: sizes around the rows of the probe
kernel and the 8 192-entry chunk of the scans, where the new hashes fall among the present ones, counts at and above
2^32, where the state came from, and several parts in one call.  The reference is union_parts of fold_restatement.py
(checked against the C oracle by test_fold_rules.py); everything is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import fold_restatement as FR

pytestmark = pytest.mark.gpu

U64 = np.uint64
TOP = (1 << 64) - 1
BIG = np.array([1, (1 << 32) - 1, 1 << 32, 1 << 40], dtype=U64)     # sums of two of them cross 2^32 or stay far from it
SIZES = [0, 1, 255, 256, 257, 8191, 8192, 8193, 16385]


def _count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U64).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(U64)


def _sketch(pkg, track):
    return pkg.KmerMinHash(0, 21, False, 42, TOP, track)


def _absorb(mh, parts, gap=0):
    """parts = [(mins, abunds or None), ...] laid out in one device buffer, `gap` unused entries in front of every part"""
    starts, lens, at = [], [], 0
    for m, _ in parts:
        at += gap
        starts.append(at); lens.append(len(m))
        at += len(m)
    flat_m = np.full(at + 1, 0xDEAD, dtype=U64)
    flat_a = np.full(at + 1, 0xDEAD, dtype=U64)
    tracked = all(a is not None for _, a in parts)
    for (m, a), st in zip(parts, starts):
        flat_m[st:st + len(m)] = m
        if tracked:
            flat_a[st:st + len(m)] = a
    mh.absorb_dev(_dev(flat_m), _dev(flat_a) if tracked else None, starts, lens)


def _exported(mh, track):
    """the state through export_dev into tensors of exactly n entries"""
    import torch
    n = mh.export_dev()
    m = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    a = torch.full((n,), -1, dtype=torch.int64, device="cuda") if track else None
    assert mh.export_dev(m, a) == n
    return _host(m), (_host(a) if track else None)


def _check(pkg, mh, want, track):
    """export_dev first (nothing may come to the host for it), then the accessors"""
    before = _count(pkg, "sketch_to_host")
    got = _exported(mh, track)
    assert _count(pkg, "sketch_to_host") == before, "export_dev brought the state to the host"
    assert np.array_equal(got[0], want[0])
    if track:
        assert np.array_equal(got[1], want[1])
    assert np.array_equal(mh.mins_np(), want[0])
    if track:
        assert np.array_equal(mh.abunds_np(), want[1])


def _counts(rng, n):
    return BIG[rng.integers(0, BIG.size, size=n)]


def _universe(rng, n):
    """n distinct ascending values of [2^20, 2^64 - 2^20): room below and above for the placements"""
    lo, hi = 1 << 20, TOP - (1 << 20)
    step = (hi - lo) // max(n, 1)
    return (U64(lo) + np.arange(n, dtype=U64) * U64(step) + rng.integers(0, step, size=n, dtype=U64)).astype(U64)


def _unite_once(pkg, track, S, D, rng):
    """an empty sketch takes S (the copy path), then D (one union when both are non-empty); returns the sketch"""
    S_ab, D_ab = (_counts(rng, S.size), _counts(rng, D.size)) if track else (None, None)
    mh = _sketch(pkg, track)
    pkg.lib().smh_profile_reset()
    _absorb(mh, [(S, S_ab)])
    assert _count(pkg, "sketch_union_on_device") == 0
    _absorb(mh, [(D, D_ab)])
    assert _count(pkg, "sketch_union_on_device") == (1 if S.size and D.size else 0)
    assert _count(pkg, "sketch_to_host") == 0
    empty = np.zeros(0, dtype=U64)
    want = FR.union_parts(empty, empty if track else None, [(S, S_ab), (D, D_ab)])
    _check(pkg, mh, want, track)
    return mh, want


@pytest.mark.parametrize("track", [True, False])
@pytest.mark.parametrize("n_s", SIZES)
def test_sizes_of_the_state_and_of_the_part(n_s, track, pkg):
    """(n_s, n_d) over the cross of the sizes; about half of the smaller side is present in the other"""
    for n_d in SIZES:
        rng = np.random.default_rng(n_s * 100_003 + n_d)
        common = min(n_s, n_d) // 2
        u = _universe(rng, n_s + n_d - common)
        pick = rng.permutation(u.size)
        S = np.sort(u[pick[:n_s]])
        D = np.sort(u[pick[n_s - common:n_s - common + n_d]])
        assert S.size == n_s and D.size == n_d and np.intersect1d(S, D).size == common
        _unite_once(pkg, track, S, D, rng)


def _placement(name, n_s, n_d, rng):
    u = _universe(rng, n_s + n_d)
    if name == "below":
        return u[n_d:], u[:n_d]
    if name == "above":
        return u[:n_s], u[n_s:]
    if name == "present":              # every hash of the part is in the state already: nothing new
        if n_d > n_s:
            n_s, n_d = n_d, n_s        # (the part cannot be larger than a state that holds all of it: the sizes change sides)
        S = u[:n_s]
        return S, np.sort(rng.choice(S, size=n_d, replace=False))
    if name == "alternating":
        k = 2 * min(n_s, n_d)
        S, D = u[0:k:2], u[1:k:2]
        rest = u[k:]
        return (np.concatenate([S, rest]), D) if n_s > n_d else (S, np.concatenate([D, rest]))
    if name == "one_gap":              # all of the part between two neighbours of the state
        at = n_s // 3
        return np.concatenate([u[:at], u[at + n_d:]]), u[at:at + n_d]
    if name == "superset":             # the part holds every hash of the state and more
        if n_d < n_s:
            n_s, n_d = n_d, n_s
        D = u[:n_d]
        return np.sort(rng.choice(D, size=n_s, replace=False)), D
    if name == "extremes":             # 0 and 2^64 - 1 are members: one on each side, and both in both
        rng.shuffle(u)
        S, D = np.sort(u[:n_s]), np.sort(u[n_s:])
        S[0], D[-1] = 0, TOP
        return S, D
    raise AssertionError(name)


@pytest.mark.parametrize("track", [True, False])
@pytest.mark.parametrize("n_s,n_d", [(8191, 8193), (257, 255)])
@pytest.mark.parametrize("name", ["below", "above", "present", "alternating", "one_gap", "superset", "extremes"])
def test_where_the_new_hashes_fall(name, n_s, n_d, track, pkg):
    """all new hashes below the state's first / above its last (the last mark, index n_s), none new, every other one,
    thousands in one gap (one mark takes every atomicAdd), the part a superset of the state, and the extreme values"""
    rng = np.random.default_rng(n_s + len(name))
    S, D = _placement(name, n_s, n_d, rng)
    assert {S.size, D.size} == {n_s, n_d} and (np.diff(S.astype(object)) > 0).all() and (np.diff(D.astype(object)) > 0).all()
    mh, want = _unite_once(pkg, track, S, D, rng)
    n_new = want[0].size - S.size
    assert n_new == {"below": D.size, "above": D.size, "present": 0, "alternating": D.size, "one_gap": D.size,
                     "superset": D.size - S.size, "extremes": D.size}[name]
    if name == "extremes":             # and once more with both extremes in the part and in the state
        both = np.array([0, TOP], dtype=U64)
        ab = _counts(rng, 2) if track else None
        _absorb(mh, [(both, ab)])
        _check(pkg, mh, FR.union_parts(want[0], want[1], [(both, ab)]), track)


def test_a_tracked_sketch_refuses_a_part_without_abundances(pkg):
    rng = np.random.default_rng(5)
    u = _universe(rng, 600)
    for filled in (False, True):
        mh = _sketch(pkg, True)
        if filled:
            _absorb(mh, [(u[:300], _counts(rng, 300))])
        with pytest.raises(pkg.SourmashError) as ei:
            _absorb(mh, [(u[200:], None)])
        assert "carries no abundances" in ei.value.message
        assert len(mh) == (300 if filled else 0)
    # an untracked sketch ignores abundances that come along
    mh = _sketch(pkg, False)
    _absorb(mh, [(u[:300], _counts(rng, 300))]); _absorb(mh, [(u[200:], _counts(rng, 400))])
    assert np.array_equal(mh.mins_np(), u) and mh.abunds_np() is None


@pytest.mark.parametrize("track", [True, False])
@pytest.mark.parametrize("origin", ["small_fold", "general_fold", "host", "absorbed"])
def test_where_the_state_comes_from(origin, track, pkg):
    """a sketch just filled by add_many holds run STARTS (the first union turns them into counts; export_dev does the same
    on the fly), one whose .mins was read lives on the host and goes back to HBM, one already absorbed into holds counts"""
    rng = np.random.default_rng(len(origin))
    u = _universe(rng, 30_000)
    n_first = {"small_fold": 5_000, "general_fold": 12_000, "host": 5_000, "absorbed": 5_000}[origin]
    first = np.sort(rng.choice(u, size=n_first, replace=False))
    empty = np.zeros(0, dtype=U64)
    mh = _sketch(pkg, track)
    pkg.lib().smh_profile_reset()
    if origin == "absorbed":
        first_ab = _counts(rng, n_first) if track else None
        _absorb(mh, [(first[:2_000], None if first_ab is None else first_ab[:2_000])])
        _absorb(mh, [(first[1_000:], None if first_ab is None else first_ab[1_000:])])
        state = FR.union_parts(empty, empty if track else None, [(first[:2_000], None if first_ab is None else first_ab[:2_000]),
                                                                   (first[1_000:], None if first_ab is None else first_ab[1_000:])])
        assert _count(pkg, "sketch_union_on_device") == 1
    else:
        stream = np.concatenate([first, first[::3], first[::7]])      # abundances 1, 2 and 3
        rng.shuffle(stream)
        mh.add_many(stream)
        assert _count(pkg, "small_fold") == (1 if origin != "general_fold" else 0)
        state = FR.scaled_add(empty, empty, stream, TOP, track)
        if origin == "host":
            assert np.array_equal(mh.mins_np(), state[0])
            assert _count(pkg, "sketch_to_host") == 1
        else:
            got = _exported(mh, track)                                # run starts -> counts inside export_dev
            assert np.array_equal(got[0], state[0]) and (not track or np.array_equal(got[1], state[1]))
            assert _count(pkg, "sketch_to_host") == 0
        assert _count(pkg, "sketch_union_on_device") == 0
    before = _count(pkg, "sketch_union_on_device")
    to_host = _count(pkg, "sketch_to_host")
    part = np.sort(rng.choice(u, size=8_193, replace=False))
    part_ab = _counts(rng, part.size) if track else None
    _absorb(mh, [(part, part_ab)])
    assert _count(pkg, "sketch_union_on_device") == before + 1 and _count(pkg, "sketch_to_host") == to_host
    want = FR.union_parts(state[0], state[1], [(part, part_ab)])
    assert np.intersect1d(state[0], part).size > 500 and want[0].size > state[0].size + 500
    _check(pkg, mh, want, track)
    assert _count(pkg, "sketch_to_host") == to_host + 1              # the accessors of _check, once


@pytest.mark.parametrize("track", [True, False])
@pytest.mark.parametrize("into", ["empty", "filled"])
def test_several_parts_in_one_call(into, track, pkg):
    """lengths [0, 1, 257, 0, 8 193] with gaps between the parts and overlapping content: the result does not depend on the
    order and equals the model; one union per non-empty part that meets a non-empty state"""
    rng = np.random.default_rng(77)
    u = _universe(rng, 12_000)
    parts = []
    for n in (0, 1, 257, 0, 8_193):
        m = np.sort(rng.choice(u, size=n, replace=False))
        parts.append((m, _counts(rng, n) if track else None))
    empty = np.zeros(0, dtype=U64)
    state = (empty, empty if track else None)
    if into == "filled":
        m0 = np.sort(rng.choice(u, size=4_000, replace=False))
        state = (m0, _counts(rng, m0.size) if track else None)
    results = []
    for order in (parts, parts[::-1]):
        mh = _sketch(pkg, track)
        if into == "filled":
            _absorb(mh, [state])
        pkg.lib().smh_profile_reset()
        _absorb(mh, order, gap=13)
        assert _count(pkg, "sketch_union_on_device") == (3 if into == "filled" else 2)
        assert _count(pkg, "sketch_to_host") == 0
        want = FR.union_parts(state[0], state[1], order)
        _check(pkg, mh, want, track)
        results.append(want)
    assert np.array_equal(results[0][0], results[1][0]) and (not track or np.array_equal(results[0][1], results[1][1]))
    assert results[0][0].size > 8_193
