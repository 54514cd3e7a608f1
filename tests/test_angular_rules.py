"""The angular similarity's rules (include/sourmash_amd.h, "Angular similarity") on the CPU: the plain-Python restatement
on hand-worked cases, the counts that pin the committed 100-sketch fixture, and the library's checks that need no device."""
import ctypes as C
import math

import pytest

import angular_restatement as AR

M64 = (1 << 64) - 1


def test_disjoint_and_identical():
    assert AR.pair({1: 3, 2: 4}, {5: 1, 6: 2}) == (0, 25, 5, 0.0, 0.0)
    # norm2 = 25: sqrt(25) * sqrt(25) is 25 exactly, the cosine is 1.0 without the clamp
    assert AR.pair({1: 3, 2: 4}, {1: 3, 2: 4}) == (25, 25, 25, 1.0, 1.0)
    # norm2 = 2: sqrt(2) * sqrt(2) rounds to 2.0000000000000004 -- the literal rule gives 1 - 2^-52, not 1.0
    d, na, nb, c, a = AR.pair({1: 1, 2: 1}, {1: 1, 2: 1})
    assert (d, na, nb) == (2, 2, 2) and 1.0 - 2.0 ** -51 <= c <= 1.0 and a > 1.0 - 1e-7
    # a product of square roots that rounds below the dot: the clamp
    assert AR.cosine_of(10, 10, 10) <= 1.0
    assert AR.cosine_of(3, 1, 1) == 1.0 and AR.angular_of(1.0) == 1.0


def test_worked_half():
    d, na, nb, c, a = AR.pair({1: 1, 2: 1}, {1: 1})
    assert (d, na, nb) == (1, 2, 1)
    assert abs(c - 1 / math.sqrt(2)) <= 1e-15
    assert abs(a - 0.5) <= 1e-15


def test_scaling_and_symmetry():
    a = {1: 2, 5: 7, 9: 1, 11: 4}
    b = {1: 3, 5: 1, 10: 6, 11: 2}
    base = AR.angular(a, b)
    assert 0.0 < base < 1.0
    for k in (2, 4, 1024):        # powers of two scale every intermediate exactly
        assert AR.angular({h: k * v for h, v in a.items()}, b) == base
        assert AR.angular(a, {h: k * v for h, v in b.items()}) == base
    assert abs(AR.angular({h: 3 * v for h, v in a.items()}, b) - base) <= 1e-15
    assert AR.pair(a, b)[0] == AR.pair(b, a)[0] == 2 * 3 + 7 * 1 + 4 * 2
    assert AR.pair(a, b)[3:] == AR.pair(b, a)[3:]


def test_empty_is_no_error():
    assert AR.pair({}, {1: 2}) == (0, 0, 4, 0.0, 0.0)
    assert AR.pair({}, {}) == (0, 0, 0, 0.0, 0.0)
    D, Cs, A = AR.block([{}, {1: 3}], [{}, {1: 3}], symmetric=True)
    assert D == [[0, 0], [0, 9]] and Cs == [[0.0, 0.0], [0.0, 1.0]] and A == Cs


def test_norm2_overflow():
    assert AR.norm2({7: (1 << 32) - 1}) == ((1 << 32) - 1) ** 2
    with pytest.raises(AR.Norm2Overflow):
        AR.norm2({7: 1 << 32})
    with pytest.raises(AR.Norm2Overflow):
        AR.norm2({7: (1 << 32) - 1, 8: (1 << 32) - 1})
    with pytest.raises(AR.Norm2Overflow):
        AR.pair({1: 1}, {1: 1 << 32})


def test_fixture_counts(sbt_subset_sketches):
    """what the GPU test of the 100 x 100 matrix leans on"""
    S = [dict(zip(s["mins"], s["abundances"])) for s in sbt_subset_sketches]
    assert len(S) == 100 and min(map(len, S)) == 314 and max(map(len, S)) == 16140
    sharing = weighted = 0
    for i in range(100):
        for j in range(i + 1, 100):
            a, b = (S[i], S[j]) if len(S[i]) <= len(S[j]) else (S[j], S[i])
            common = sum(1 for h in a if h in b)
            if common:
                sharing += 1
                weighted += AR.dot(a, b) != common
    assert sharing == 1398
    assert weighted == 745


# ---------------------------------------------------------------------------------- the library, without a device

def mk(pkg, items, track=True, ksize=21, seed=42, max_hash=M64, protein=False):
    mh = pkg.KmerMinHash(0, ksize, protein, seed, max_hash, track)
    for h, a in items:
        for _ in range(a if track else 1):
            mh.add_hash(h)          # host code: no device
    return mh


def pair_code(pkg, a, b):
    out = [C.c_double(7.0), C.c_double(7.0)]
    ints = [C.c_uint64(7) for _ in range(3)]
    code = pkg.lib().smh_angular_similarity(a._p, b._p, C.byref(out[0]), C.byref(out[1]), *[C.byref(x) for x in ints])
    untouched = all(x.value == 7.0 for x in out) and all(x.value == 7 for x in ints)
    pkg.lib().sourmash_err_clear()
    return code, untouched


def test_symbols_are_exported(pkg):
    want = {"smh_index_has_abundances", "smh_index_norms2", "smh_index_angular", "smh_index_angular_query", "smh_angular_similarity",
            "smh_angular_block_dev", "smh_angular_last_stats"}
    assert want <= set(pkg.exported_symbols())
    assert 1 <= pkg.lib().smh_angular_prune_min_pairs() <= 10_000
    for name in ("angular_similarity", "similarity"):
        assert hasattr(pkg.KmerMinHash, name)
    for name in ("has_abundances", "norms2", "angular", "angular_matrix"):
        assert hasattr(pkg.index.ResidentIndex, name)
    assert hasattr(pkg.matrix, "angular_block_dev")


def test_pair_checks_come_before_the_device(pkg):
    """the same codes with and without a GPU: nothing is launched for a pair that is refused"""
    a = mk(pkg, [(1, 2), (5, 1)])
    flat = mk(pkg, [(1, 1), (5, 1)], track=False)
    for x, y in ((a, flat), (flat, a), (flat, flat)):
        assert pair_code(pkg, x, y) == (3, True)
    with pytest.raises(pkg.SourmashError) as ei:
        a.angular_similarity(flat)
    assert ei.value.code == 3 and "does not track abundances" in ei.value.message
    for code, kw in ((101, dict(ksize=31)), (102, dict(protein=True)), (103, dict(max_hash=1 << 62)), (104, dict(seed=43))):
        other = mk(pkg, [(1, 2)], **kw)
        assert pair_code(pkg, a, other) == (code, True), kw
        assert pair_code(pkg, other, a) == (code, True), kw
    # similarity(): angular only when both track abundances and it is not switched off; a refusal of the pair stays one
    with pytest.raises(pkg.SourmashError) as ei:
        a.similarity(mk(pkg, [(1, 2)], seed=43))
    assert ei.value.code == 104
    if not pkg.device_available():
        with pytest.raises(pkg.SourmashError) as ei:
            a.angular_similarity(a)            # an accepted pair needs the device, and says so
        assert ei.value.code == 2


def test_index_checks(pkg):
    """an index with one node that tracks no abundances: has_abundances is false and the angular calls are refused.  A
    resident index lives in HBM, so without a device there is none to ask: its construction says so (code 2)."""
    a, b = mk(pkg, [(1, 2), (5, 1)]), mk(pkg, [(1, 1), (7, 3)])
    flat = mk(pkg, [(1, 1), (5, 1)], track=False)
    L = pkg.lib()
    assert L.smh_index_has_abundances(None) is False
    if not pkg.device_available():
        with pytest.raises(pkg.SourmashError) as ei:
            pkg.index.ResidentIndex([a, flat])
        assert ei.value.code == 2
        return
    mixed = pkg.index.ResidentIndex([a, flat, b])
    full = pkg.index.ResidentIndex([a, b])
    assert mixed.has_abundances is False and full.has_abundances is True
    assert L.smh_index_has_abundances(mixed._h) is False and L.smh_index_has_abundances(full._h) is True
    import numpy as np
    dot = np.full(9, 7, np.uint64)
    assert L.smh_index_angular(mixed._h, mixed._h, dot.ctypes.data_as(pkg._lib.u64p), None, None) == 3
    L.sourmash_err_clear()
    assert (dot == 7).all()
    for call in (lambda: mixed.angular_matrix(), lambda: mixed.angular_matrix(full), lambda: full.angular_matrix(mixed),
                 lambda: mixed.norms2(), lambda: mixed.angular(a), lambda: full.angular(flat)):
        with pytest.raises(pkg.SourmashError) as ei:
            call()
        assert ei.value.code == 3 and "angular" in ei.value.message
    assert mixed.find(a, 0.4) == [0, 1]          # such an index still serves find
