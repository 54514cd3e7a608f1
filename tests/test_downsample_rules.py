"""The rules of downsampling (include/sourmash_amd.h, "Downsampling") without a GPU: the restatement against
both oracles, max_hash <-> scaled, and the library's host path (sketches filled by mins_push / abunds_push) against the
restatement, refusals included."""
import random

import pytest

import downsample_restatement as R

MX = 1 << 60


def _state(rng, n, track):
    mins = sorted(rng.sample(range(1, MX), n))
    return mins, ([rng.randint(1, 9) for _ in mins] if track else None)


def _cuts(mins):
    """new max_hash values: on a hash (kept), just below it (dropped), below everything, above everything, the old value"""
    mid = mins[len(mins) // 2]
    return [mid, mid - 1, mins[0], mins[0] - 1, mins[-1], mins[-1] + 1, MX]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("which", ["coracle", "pyoracle"])
def test_restatement_agrees_with_the_oracles(request, which, track):
    oracle = request.getfixturevalue(which)
    rng = random.Random(5)
    mins, abunds = _state(rng, 200, track)
    for new in _cuts(mins):
        fresh = oracle.MinHash(0, 21, False, 42, new, track)
        if track:
            fresh.add_many_with_abund(list(zip(mins, abunds)))
        else:
            fresh.add_many(mins)
        want_m, want_a = R.cut(mins, abunds, new)
        assert list(fresh.mins) == want_m
        assert (list(fresh.abunds) if track else None) == want_a
    mid = mins[100]
    assert R.cut(mins, abunds, mid)[0][-1] == mid and R.cut(mins, abunds, mid - 1)[0][-1] == mins[99]


def test_max_hash_of_scaled_inverts_scaled_of_max_hash(pkg):
    from sourmash_rust_amd.index import max_hash_of_scaled, scaled_of_max_hash
    for s in [1, 2, 3, 10, 100, 1000, 2000, 10 ** 6] + list(range(1, 10 ** 6, 7919)):
        assert max_hash_of_scaled(s) == R.max_hash_of_scaled(s) == min((1 << 64) // s, (1 << 64) - 1)
        assert scaled_of_max_hash(max_hash_of_scaled(s)) == s
    assert max_hash_of_scaled(1) == (1 << 64) - 1


def _sketch(pkg, num, mx, mins, abunds, **kw):
    mh = pkg.KmerMinHash(num, kw.get("ksize", 21), kw.get("prot", False), kw.get("seed", 42), mx, abunds is not None)
    for h in mins:
        mh.mins_push(h)
    for a in abunds or []:
        mh.abunds_push(a)
    return mh


def _params(mh):
    return mh.num, mh.ksize, mh.is_protein, mh.molecule, mh.seed, mh.track_abundance


@pytest.mark.parametrize("track", [False, True])
def test_host_max_hash_cut_equals_the_restatement(pkg, track):
    rng = random.Random(9)
    mins, abunds = _state(rng, 300, track)
    src = _sketch(pkg, 0, MX, mins, abunds, ksize=31, seed=7)
    for new in _cuts(mins):
        got = src.downsample_max_hash(new)
        _, want_mx, want_m, want_a = R.downsample_max_hash(0, MX, mins, abunds, new)
        assert (got.max_hash, got.mins, got.abunds) == (want_mx, want_m, want_a)
        assert _params(got) == _params(src)
    assert (src.mins, src.abunds, src.max_hash) == (mins, abunds, MX)   # the source is left alone
    # through scaled, and the scaled property
    s = src.downsample_scaled(1000)
    assert s.max_hash == R.max_hash_of_scaled(1000) and s.scaled == 1000
    assert s.mins == R.cut(mins, abunds, s.max_hash)[0]
    assert pkg.KmerMinHash(5, 21).scaled is None


def test_equal_max_hash_gives_an_equal_independent_copy(pkg):
    mins, abunds = _state(random.Random(2), 50, True)
    src = _sketch(pkg, 0, MX, mins, abunds)
    cp = src.downsample_max_hash(MX)
    assert (cp.mins, cp.abunds, cp.max_hash, _params(cp)) == (mins, abunds, MX, _params(src))
    cp.add_hash(mins[0])
    src.add_hash(mins[1])
    assert cp.abunds[0] == abunds[0] + 1 and cp.abunds[1] == abunds[1]
    assert src.abunds[0] == abunds[0] and src.abunds[1] == abunds[1] + 1


@pytest.mark.parametrize("track", [False, True])
def test_host_num_cut_equals_the_restatement(pkg, track):
    mins, abunds = _state(random.Random(4), 40, track)
    src = _sketch(pkg, 40, 0, mins, abunds)
    for new in (1, 7, 39, 40):
        got = src.downsample_num(new)
        want_num, _, want_m, want_a = R.downsample_num(40, 0, mins, abunds, new)
        assert (got.num, got.max_hash, got.mins, got.abunds) == (want_num, 0, want_m, want_a)
        assert _params(got)[1:] == _params(src)[1:]
    short = _sketch(pkg, 100, 0, mins, abunds)   # fewer hashes than the new num: all of them
    assert short.downsample_num(60).mins == mins and short.downsample_num(60).num == 60


def test_refusals_are_msg_and_name_the_values(pkg):
    mins, abunds = _state(random.Random(6), 10, True)
    scaled = _sketch(pkg, 0, MX, mins, abunds)
    num = _sketch(pkg, 10, 0, mins, abunds)
    both = _sketch(pkg, 10, MX, mins, abunds)       # num and max_hash: not a scaled sketch, not a num sketch
    neither = _sketch(pkg, 0, 0, mins, abunds)
    cases = [(lambda: scaled.downsample_max_hash(0), (0, MX, 0), ["0"]),
             (lambda: scaled.downsample_max_hash(MX + 1), (0, MX, MX + 1), [str(MX + 1), str(MX)]),
             (lambda: num.downsample_max_hash(5), (10, 0, 5), ["10"]),
             (lambda: both.downsample_max_hash(5), (10, MX, 5), ["10", str(MX)]),
             (lambda: neither.downsample_max_hash(5), (0, 0, 5), ["0"])]
    for fn, (n, mx, new), words in cases:
        with pytest.raises(R.Refused):
            R.downsample_max_hash(n, mx, mins, abunds, new)
        with pytest.raises(pkg.SourmashError) as ei:
            fn()
        assert ei.value.code == 3
        assert all(w in ei.value.message for w in words), ei.value.message
    cases = [(lambda: num.downsample_num(0), (10, 0, 0), ["0"]),
             (lambda: num.downsample_num(11), (10, 0, 11), ["11", "10"]),
             (lambda: scaled.downsample_num(1), (0, MX, 1), [str(MX)]),
             (lambda: both.downsample_num(5), (10, MX, 5), [str(MX)])]
    for fn, (n, mx, new), words in cases:
        with pytest.raises(R.Refused):
            R.downsample_num(n, mx, mins, abunds, new)
        with pytest.raises(pkg.SourmashError) as ei:
            fn()
        assert ei.value.code == 3
        assert all(w in ei.value.message for w in words), ei.value.message
    assert pkg.lib().sourmash_err_get_last_code() == 0


def test_common_max_hash_is_the_smaller_of_two_scaled(pkg):
    assert R.common_max_hash(0, 100, 0, 70) == 70 == R.common_max_hash(0, 70, 0, 100)
    for bad in ((5, 0, 0, 70), (0, 70, 5, 70), (0, 0, 0, 70)):
        with pytest.raises(R.Refused):
            R.common_max_hash(*bad)
