"""The fold behind add_many at the sizes where its branches change: the two one-workgroup small folds and what happens when
they decline, run boundaries against the small fold's slot ownership and against the tiles, rows and waves of the
run-length encoding, the bottom-num twin, the 8-byte payload sorts, and the hand-over of merge to the device.

Every case drives the ACTUAL candidate count to an exact value with plain integer arrays (add_many of 4 096 or more hashes
goes through the same ingest as sequences), is bit-exact against the numpy model of fold_restatement.py or the C oracle,
and asserts by route counter that the branch it aims at ran.  The thresholds are the ones the library documents:

    small fold, half instance   expected <= 5 734,   takes up to  8 192 candidates
    small fold, full instance   expected <  11 468.8, takes up to 16 384 candidates
    candidate buffer            1.25 * expected + 65 536 entries (at most one per hash)
    one-workgroup sort          up to 8 192 keys
    merge on the device         from 65 536 combined hashes"""
import ctypes as C

import numpy as np
import pytest

import fold_restatement as FR

pytestmark = pytest.mark.gpu

U64 = np.uint64
TOP = (1 << 64) - 1
ROUTES = ("small_fold", "small_fold_passed_on", "small_fold_overflow", "chunk_rerun")
EMPTY = (np.zeros(0, dtype=U64), np.zeros(0, dtype=U64))


def _count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


def _routes(pkg, names=ROUTES):
    return {n: _count(pkg, n) for n in names}


def _route(**kw):
    out = dict.fromkeys(ROUTES, 0)
    out.update(kw)
    return out


def _spread(rng, n, lo, hi):
    """n DISTINCT values of [lo, hi], ascending: one from every n-th of the range"""
    if n == 0:
        return np.zeros(0, dtype=U64)
    step = min((hi - lo + 1) // n, 1 << 63)
    assert step >= 1
    return (U64(lo) + np.arange(n, dtype=U64) * U64(step) + rng.integers(0, step, size=n, dtype=U64)).astype(U64)


def _pinned(rng, P, N, max_hash):
    """P distinct hashes, shuffled, exactly N of them <= max_hash"""
    a = np.concatenate([_spread(rng, N, 0, max_hash), _spread(rng, P - N, max_hash + 1, TOP) if P > N else np.zeros(0, dtype=U64)])
    rng.shuffle(a)
    return a


def _from_runs(rng, lengths, lo, hi):
    """a shuffled array whose sorted multiset has runs of these lengths, in this order; the keys lie in [lo, hi]"""
    keys = _spread(rng, len(lengths), lo, hi)
    a = np.repeat(keys, np.asarray(lengths, dtype=np.int64))
    rng.shuffle(a)
    return a


def _check_scaled(pkg, g, want, track):
    assert np.array_equal(g.mins_np(), want[0])
    if track:
        assert np.array_equal(g.abunds_np(), want[1])


def _add_into_empty(pkg, hashes, max_hash, track, route):
    g = pkg.KmerMinHash(0, 21, False, 42, max_hash, track)
    pkg.lib().smh_profile_reset()
    g.add_many(hashes)
    assert _routes(pkg) == route
    _check_scaled(pkg, g, FR.scaled_add(EMPTY[0], EMPTY[1] if track else None, hashes, max_hash, track), track)
    return g


# ---------------------------------------------------------------------------------------------------------------------
# scaled, into an empty sketch, the actual count pinned

HALF = (100_000, (1 << 64) // 25)     # 4 000 expected: the half instance, well inside its band
FULL = (100_000, (1 << 64) // 12)     # 8 333 expected: the full instance

PINNED = ([(HALF, n, "small_fold") for n in (0, 1, 1023, 1024, 1025, 5734, 8191, 8192)] + [(HALF, 8193, "small_fold_passed_on")] +
          [(FULL, n, "small_fold") for n in (8193, 11468, 16383, 16384)] + [(FULL, 16385, "small_fold_passed_on")])


@pytest.mark.parametrize("track", [True, False])
@pytest.mark.parametrize("shape,N,route", PINNED, ids=["%s-%d" % ("half" if s is HALF else "full", n) for s, n, _ in PINNED])
def test_scaled_small_fold_takes_up_to_its_capacity_and_hands_on_above(shape, N, route, track, pkg):
    """exactly N of the P hashes pass the threshold: up to the instance's capacity the small fold is the whole fold; one
    more and it declines, and the general path reuses the candidates that are already in the buffer (no second hashing)"""
    P, max_hash = shape
    rng = np.random.default_rng(1000 + N)
    g = _add_into_empty(pkg, _pinned(rng, P, N, max_hash), max_hash, track, _route(**{route: 1}))
    assert len(g) == N


@pytest.mark.parametrize("track", [True, False])
@pytest.mark.parametrize("max_hash", [(1 << 64) // 50, (1 << 64) // 25], ids=["half", "full"])
def test_scaled_small_fold_overflows_its_buffer(max_hash, track, pkg):
    """P = 200 000 with 4 000 / 8 000 expected: the buffer holds 70 536 / 75 536, and 90 000 hashes pass.  The small fold
    reports the overflow and the hashing is run again by the general path, which sizes its buffer by the count the first
    launch left behind: chunk_rerun == 0, two hashing passes.  (Before these tests the general path started from the same
    estimate again, overflowed again and only its re-run was kept: chunk_rerun == 1, three passes.)"""
    rng = np.random.default_rng(90)
    _add_into_empty(pkg, _pinned(rng, 200_000, 90_000, max_hash), max_hash, track, _route(small_fold_overflow=1))


@pytest.mark.parametrize("P", [4096, 5734, 5735, 11468, 11469])
def test_everything_passes_at_the_expected_counts_that_choose_the_path(P, pkg):
    """max_hash = 2^64 - 1: expected == actual == P.  5 734 / 5 735 is the choice of instance, 11 468 / 11 469 the end of the
    small fold (the last one never enters it)"""
    rng = np.random.default_rng(P)
    hashes = _pinned(rng, P, P, TOP)
    for track in (True, False):
        _add_into_empty(pkg, hashes, TOP, track, _route(small_fold=1) if P <= 11468 else _route())


@pytest.mark.parametrize("N", [5000, 8192, 11468, 12000])
def test_the_smallest_and_the_largest_hash_are_members(N, pkg):
    """0 and 2^64 - 1 (the value the small fold pads its slots with) among the hashes, both twice"""
    rng = np.random.default_rng(N)
    hashes = np.concatenate([_spread(rng, N - 4, 1, TOP - 1), np.array([0, 0, TOP, TOP], dtype=U64)])
    rng.shuffle(hashes)
    g = _add_into_empty(pkg, hashes, TOP, True, _route(small_fold=1) if N <= 11468 else _route())
    assert g.mins[0] == 0 and g.mins[-1] == TOP and g.abunds[0] == 2 and g.abunds[-1] == 2 and len(g) == N - 2


# ---------------------------------------------------------------------------------------------------------------------
# runs against the small fold's slot ownership: thread t owns `items` consecutive sorted slots, items = ceil(N / 1024)

def _small_fold_runs(pkg, rng, lengths):
    """tracked, through the small fold: N = sum(lengths) candidates among P = 100 000 hashes"""
    N = int(np.sum(lengths))
    P, max_hash = HALF if N <= 8192 else FULL
    low = _from_runs(rng, lengths, 0, max_hash)
    hashes = np.concatenate([low, _spread(rng, P - N, max_hash + 1, TOP)])
    rng.shuffle(hashes)
    g = _add_into_empty(pkg, hashes, max_hash, True, _route(small_fold=1))
    assert np.array_equal(g.abunds_np(), np.asarray(lengths, dtype=U64))
    return g


@pytest.mark.parametrize("N", [8000, 8192, 16000, 16384])
def test_small_fold_one_key_5000_times_among_distinct_ones(N, pkg):
    rng = np.random.default_rng(N)
    for where in (0, (N - 5000) // 2, N - 5000):               # the long run first, in the middle, last
        lengths = [1] * where + [5000] + [1] * (N - 5000 - where)
        _small_fold_runs(pkg, rng, lengths)


@pytest.mark.parametrize("N", [3 * 341, 3 * 342, 3 * 2730, 3 * 5461])
def test_small_fold_every_key_three_times(N, pkg):
    _small_fold_runs(pkg, np.random.default_rng(N), [3] * (N // 3))


@pytest.mark.parametrize("N", [1, 1024, 1025, 8192, 8193, 16384])
def test_small_fold_all_candidates_equal(N, pkg):
    g = _small_fold_runs(pkg, np.random.default_rng(N), [N])
    assert len(g) == 1


@pytest.mark.parametrize("items", [1, 2, 8, 16])
@pytest.mark.parametrize("fill", ["full", "short"])
def test_small_fold_runs_that_end_and_start_at_a_threads_first_slot(items, fill, pkg):
    """runs of items + 1 keys (longer than what one thread owns) that END at slot items * t - 1, and runs that START at slot
    items * t, for threads at the start, at wave boundaries and at the end of the workgroup; single keys in between.
    fill = short: the last thread's slots are not all used"""
    N = items * 1024 - (0 if fill == "full" else items // 2 + 1)
    L = items + 1
    ends = [items * t for t in (2, 64, 128, 512, 1022)]         # a run occupies [e - L, e)
    begins = [items * t for t in (5, 192, 320, 640, 1023)]       # a run occupies [b, min(b + L, N))
    spans = sorted([(e - L, e) for e in ends] + [(b, min(b + L, N)) for b in begins])
    lengths, at = [], 0
    for lo, hi in spans:
        if hi <= lo:
            continue                                             # (fill = short with one slot per thread: the last thread has none)
        assert lo >= at and hi <= N
        lengths += [1] * (lo - at) + [hi - lo]
        at = hi
    lengths += [1] * (N - at)
    assert sum(lengths) == N and (N + 1023) // 1024 == items
    _small_fold_runs(pkg, np.random.default_rng(items), lengths)


# ---------------------------------------------------------------------------------------------------------------------
# run boundaries against the geometry of the run-length encoding (general path): tiles of 2 048, rows of 256, waves of 64

EDGES = [63, 1, 1, 190, 1, 1, 1790, 1, 1]      # run boundaries at 63 / 64 / 65, 255 / 256 / 257, 2 047 / 2 048 / 2 049
THREE_TILES = 8196                              # from 2 049 to 10 245: the tiles [4 096, 10 240) hold no run head
RLE_CASES = {
    "8192-last1": EDGES + [1] * (8192 - 2049),
    "8193-last1": EDGES + [1] * (8193 - 2049),
    "8193-last2": EDGES + [1] * (8193 - 2049 - 2) + [2],
    "7x2048-1-last2049": EDGES + [THREE_TILES] + [1] * (7 * 2048 - 1 - 10245 - 2049) + [2049],
    "7x2048+1-last1": EDGES + [THREE_TILES] + [1] * (7 * 2048 + 1 - 10245),
    "6x2048-last2049": EDGES + [1] * (6 * 2048 - 2049 - 2049) + [2049],     # the last run starts one before a tile does
}


@pytest.mark.parametrize("case", sorted(RLE_CASES))
def test_run_boundaries_against_the_tiles_of_the_run_length_encoding(case, pkg):
    """a tracked scaled sketch that already holds hashes (so the small fold is out of the way) takes a batch whose sorted
    candidates have these runs: the batch goes through the sort and the run-length encoding.  add_many brings the state to
    the host first (sketch_to_host == 1), so the batch's distinct hashes and run starts are read back and merged there, not
    united on the device.  Half of the batch's keys are present in the sketch already, so run lengths are both inserted
    and added"""
    lengths = RLE_CASES[case]
    total = sum(lengths)
    rng = np.random.default_rng(total)
    keys = _spread(rng, len(lengths), 0, TOP) & ~U64(1)                  # the batch's keys are even, ascending, distinct
    first = np.concatenate([keys[::2], _spread(rng, 4096, 0, TOP) | U64(1)])   # the sketch holds every other one, and odd ones
    rng.shuffle(first)
    batch = np.repeat(keys, np.asarray(lengths, dtype=np.int64))
    assert batch.size == total
    rng.shuffle(batch)
    g = pkg.KmerMinHash(0, 21, False, 42, TOP, True)
    g.add_many(first)
    pkg.lib().smh_profile_reset()
    g.add_many(batch)
    assert _routes(pkg) == _route()
    assert _count(pkg, "sketch_to_host") == 1 and _count(pkg, "sketch_union_on_device") == 0
    want = FR.scaled_add(*FR.scaled_add(EMPTY[0], EMPTY[1], first, TOP, True), batch, TOP, True)
    _check_scaled(pkg, g, want, True)
    assert int(want[1].max()) >= max(lengths)


# ---------------------------------------------------------------------------------------------------------------------
# num mode

def _num_array(rng, D, r, P=200_000):
    """D distinct values below 2^40, each r times, the rest distinct above 2^63; shuffled"""
    a = np.concatenate([np.repeat(_spread(rng, D, 0, (1 << 40) - 1), r), _spread(rng, P - D * r, 1 << 63, TOP)])
    assert a.size == P
    rng.shuffle(a)
    return a


NUM_CASES = [
    # num, D, r, route
    (2835, 2836, 1, "small_fold"), (2836, 2837, 1, "small_fold"),
    (2835, 4097, 2, "small_fold_passed_on"),          # 8 194 candidates: the half instance (2 * 2835 + 64 == 5 734) declines them
    (2836, 4097, 2, "small_fold"),                    # ... the full instance (5 736) takes them
    (5702, 5800, 1, "small_fold"), (5703, 5800, 1, None),     # 2 * num + 64 against 0.7 * 16 384: the last one is the general path
    (2836, 2835, 1, "small_fold"), (2836, 2836, 1, "small_fold"), (2836, 2837, 1, "small_fold"),   # D = num - 1: nothing applied
    (2836, 2835, 3, "small_fold"),
    (2836, 4096, 4, "small_fold"),                    # 16 384 candidates
    (2836, 3277, 5, "small_fold_passed_on"),          # 16 385: candidates reused
    (2836, 4000, 20, "small_fold_overflow"),          # 80 000 > 1.25 * 5 736 + 65 536
]


@pytest.mark.parametrize("num,D,r,route", NUM_CASES, ids=["num%d-D%d-r%d" % c[:3] for c in NUM_CASES])
def test_num_untracked_into_an_empty_sketch(num, D, r, route, pkg):
    """the bottom-num twin of the small fold.  With fewer than num distinct hashes under the estimate the small fold runs
    but nothing is applied: the growing chunks take over and the result is still the bottom-num of ALL hashes (the ones above
    2^63 included).  An overflow is hashed again by the general path into a buffer of the size the first launch counted
    (chunk_rerun == 0, as in the scaled case)."""
    rng = np.random.default_rng(num * 31 + D * r)
    hashes = _num_array(rng, D, r)
    g = pkg.KmerMinHash(num, 21, False, 42, 0, False)
    pkg.lib().smh_profile_reset()
    g.add_many(hashes)
    assert _routes(pkg) == _route(**({route: 1} if route else {}))
    model = FR.num_add_untracked(EMPTY[0], hashes, num)
    assert model.size == num and (D >= num) == bool(model[-1] < (1 << 40))
    assert np.array_equal(g.mins_np(), model)
    g.add_many(hashes[:5000])                                     # and the sketch goes on working from that state
    assert np.array_equal(g.mins_np(), model)


TRACKED_NUM = [(2000, 4096, 2), (2000, 2731, 3), (2000, 2048, 4), (2000, 1999, 4), (2000, 8192, 1), (2000, 8193, 1), (2836, 3277, 5),
               (2836, 4000, 20)]


@pytest.mark.parametrize("num,D,r", TRACKED_NUM, ids=["num%d-D%d-r%d" % c for c in TRACKED_NUM])
def test_num_tracked_against_the_oracle(num, D, r, pkg, coracle):
    """tracked bottom-num sketches are order-dependent (quirk Q3): the C oracle fed the same array is the reference.  The
    candidates carry their stream positions as an 8-byte payload: 8 192 of them are sorted by one workgroup, 8 193 by the
    radix passes (D * r = 8 192 / 8 193); then a second array into the filled sketch"""
    rng = np.random.default_rng(num + D * r)
    hashes = _num_array(rng, D, r)
    g, o = pkg.KmerMinHash(num, 21, False, 42, 0, True), coracle.MinHash(num, 21, False, 42, 0, True)
    pkg.lib().smh_profile_reset()
    g.add_many(hashes); o.add_many(hashes)
    assert _routes(pkg, ROUTES[:3]) == dict.fromkeys(ROUTES[:3], 0), "a tracked bottom-num sketch has no small fold"
    assert np.array_equal(g.mins_np(), o.mins_np()) and np.array_equal(g.abunds_np(), o.abunds_np())
    again = np.concatenate([hashes[:6000], _spread(rng, 3000, 0, (1 << 40) - 1)])
    rng.shuffle(again)
    g.add_many(again); o.add_many(again)
    assert np.array_equal(g.mins_np(), o.mins_np()) and np.array_equal(g.abunds_np(), o.abunds_np())


# ---------------------------------------------------------------------------------------------------------------------
# merge: the host loop below 65 536 combined hashes, the device from there on

@pytest.fixture(scope="module")
def merge_sides():
    """two ascending hash arrays with about 5 000 hashes in common, and abundances among 1, 2^32 - 1, 2^32, 2^40"""
    rng = np.random.default_rng(65536)
    universe = _spread(rng, 75_000, 0, (1 << 62) - 1)
    pick = rng.permutation(universe.size)
    a = np.sort(universe[pick[:33_000]])
    b_all = np.sort(universe[pick[28_000:28_000 + 40_000]])
    big = np.array([1, 2, (1 << 32) - 1, 1 << 32, 1 << 40], dtype=U64)
    return a, big[rng.integers(0, 5, size=a.size)], b_all, big[rng.integers(0, 5, size=b_all.size)]


def _filled(cls, num, max_hash, track, mins, abunds):
    mh = cls(num, 21, False, 42, max_hash, track)
    for h in mins.tolist():
        mh.mins_push(h)
    if track:
        for c in abunds.tolist():
            mh.abunds_push(c)
    return mh


@pytest.mark.parametrize("total", [65535, 65536, 65537, 65536 + 2048])
@pytest.mark.parametrize("num,max_hash", [(0, 1 << 62), (40_000, 0)], ids=["scaled", "num40000"])
@pytest.mark.parametrize("track", [True, False])
def test_merge_at_the_hand_over_to_the_device(track, num, max_hash, total, merge_sides, pkg, coracle):
    """both tracked (sums of 2^32 - 1, 2^32 and 2^40 on the hashes present in both) and none tracked, scaled and num = 40 000
    (the mins are cut to num, the abundances are not: quirks Q5/Q6), against the C oracle's merge"""
    a, a_ab, b_all, b_ab_all = merge_sides
    b, b_ab = b_all[:total - a.size], b_ab_all[:total - a.size]
    assert a.size + b.size == total and b.size <= 40_000 and np.intersect1d(a, b).size > 3_000
    ga, gb = (_filled(pkg.KmerMinHash, num, max_hash, track, m, c) for m, c in ((a, a_ab), (b, b_ab)))
    oa, ob = (_filled(coracle.MinHash, num, max_hash, track, m, c) for m, c in ((a, a_ab), (b, b_ab)))
    pkg.lib().smh_profile_reset()
    ga.merge(gb); oa.merge(ob)
    assert _count(pkg, "merge_on_device") == (1 if total >= 65536 else 0)
    assert ga.track_abundance
    assert np.array_equal(ga.mins_np(), oa.mins_np()) and np.array_equal(ga.abunds_np(), oa.abunds_np())
    assert len(ga) == (40_000 if num else total - np.intersect1d(a, b).size)
    if track:
        ab = oa.abunds_np()
        assert ab.size == total - np.intersect1d(a, b).size and int(ab.max()) == 1 << 41
        assert ((ab > U64(1 << 32)) & (ab < U64(1 << 33))).any()
    else:
        assert oa.abunds_np().size == 0
    assert np.array_equal(gb.mins_np(), b)                          # the other side is unchanged
