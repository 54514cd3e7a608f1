"""The three small compare paths at the sizes where their code changes ("Which small kernel serves which size"):

  pair path   k_pair_block<256> / k_pair_block<1024> / k_pair_grid   (launch_compare_pair: every pairwise call of the ABI)
  wave route  k_compare_wave<InLds>                                  (tuning route="wave")
  few route   k_compare_few<QLds, WantCC>                            (tuning route="few")

Every number is compared with `==` against pair_restatement.py, which test_pair_rules.py checks against the C oracle: the
f64 results are quotients of exactly representable integers.  The one special case is the containment of an empty sketch,
0/0, asserted as NaN.  The inputs are PR.structures(): identical, interleaved, one below the other, empty-sided and
half-overlapping sketches whose hashes span all 64 bits and hold 0, 2^63 - 1, 2^63 and 2^64 - 1; the nums put the cut of
the union walk on the boundaries of the kernels' shares of the merged sequence and around the end of the union."""
import ctypes as C

import numpy as np
import pytest

import pair_restatement as PR

pytestmark = pytest.mark.gpu

U64 = np.uint64
ALL = ("jaccard", "common", "size", "count_common", "containment")
NO_CC = ("jaccard", "common", "size")           # selects the WantCC = false instantiations (the early exit of wave_pair)


def _mh(pkg, mins, num):
    g = pkg.KmerMinHash(num, 21, False, 42, 0)
    push, p = g._L.kmerminhash_mins_push, g._p
    for h in mins.tolist():
        push(p, h)                               # raw push: the length does not depend on num
    return g


def _launches(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


def _cu_count(pkg):
    dev, cus = C.c_int(), C.c_int()
    assert pkg.lib().smh_device_info(C.byref(dev), C.byref(cus)) == 0
    return cus.value


def _cuts(a, b, share, aligned=True):
    """0 (no cut) and: 1; share - 1, share, share + 1 and the same around 64 shares, where `share` is
    what one lane takes of the MERGED sequence; the end of the union - 1, + 0, + 1.  A lane boundary is a position in the
    merged sequence, the cut a rank in the union: the ranks reached after one share and after 64 (a wave's) are added with
    their neighbours, so that the cut falls ON those boundaries whatever the share of duplicates."""
    tot_u = PR.pair(a, b, 0)[1]
    ns = {0, 1, share - 1, share, share + 1, 64 * share - 1, 64 * share, 64 * share + 1, tot_u - 1, tot_u, tot_u + 1}
    for m in (share, 64 * share) if aligned else ():
        r = PR.union_rank_of_merged_prefix(a, b, m)
        ns.update([r - 1, r, r + 1])
    return sorted(n for n in ns if n >= 0)


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _same(got, exp, names, where):
    for k in names:
        g = _np(got[k])
        if k in ("jaccard", "containment"):
            ok = (g == exp[k]) | (np.isnan(g) & np.isnan(exp[k]))
            if k == "jaccard":
                assert not np.isnan(g).any(), where
        else:
            ok = g.view(U64) == exp[k]
        assert ok.all(), (where, k, np.argwhere(~ok)[:5].tolist())


def _block(pkg, route, fn):
    """fn() under the pinned route; the route the library reports must be the pinned one"""
    with pkg.matrix.tuning(route=route):
        out = fn()
        st = pkg.matrix.last_stats()
    if route != "auto":
        assert st["route"] == route, st
    return out


def _dev(pkg, sketches):
    import torch
    flat, off = pkg.matrix.csr_from_sketches(sketches)
    assert flat.size, "a device block needs at least one hash"
    return torch.from_numpy(flat.view(np.int64)).cuda(), off


# ---------------------------------------------------------------------------------------------- pair path
# launch_compare_pair: la + lb <= 8192 -> k_pair_block<256>; above -> k_pair_block<1024>; num == 0 and la + lb > 32768 ->
# k_pair_grid.  768 and 1025 / 8193 / 39935 give the 256- and 1024-thread kernels an ODD share (3, 5 / 9 / 39): with
# identical sketches every other lane boundary then falls between a hash of A and its duplicate in B.
# (the largest size with nums takes its structures in two halves: what costs time is pushing the hashes, once per num)
PAIR_CASES = [(t, True, slice(None)) for t in (0, 1, 63, 64, 65, 255, 256, 257, 768, 1023, 1024, 1025, 8191, 8192, 8193)] + \
             [(t, False, slice(None)) for t in (32767, 32768, 32769, 39935)] + [(39935, True, slice(0, 6)), (39935, True, slice(6, None))]


@pytest.mark.parametrize("total,truncated,part", PAIR_CASES,
                         ids=["%d-%s%s" % (t, "nums" if c else "num0", "-from%d" % p.start if p.start is not None else "") for t, c, p in PAIR_CASES])
def test_pair_path(total, truncated, part, pkg):
    """Every structure with la + lb == total through compare, count_common, intersection_size, intersection and containment,
    in both orders, at every cut position (or with num 0 alone).  Every call must show as one launch under the profile name
    of launch_compare_pair: should the pairwise calls be rerouted one day, this test must not quietly check another kernel."""
    rng = np.random.default_rng(1000 + total)
    threads = 256 if total <= 8192 else 1024
    share = -(-total // threads)
    L = pkg.lib()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    calls = 0
    try:
        for name, a, b in PR.structures(total, rng)[part]:
            for n in (_cuts(a, b, share, aligned=total < 10000) if truncated else [0]):
                ga, gb = _mh(pkg, a, n), _mh(pkg, b, n)
                for (x, gx), (y, gy) in (((a, ga), (b, gb)), ((b, gb), (a, ga))):        # both orders
                    common, size, cc, jac, cont = PR.pair(x, y, n)
                    where = (name, n, x.size, y.size)
                    assert gx.intersection_size(gy) == (common, size), where
                    assert gx.count_common(gy) == cc, where
                    assert gx.compare(gy) == jac, where
                    assert gx.intersection(gy) == size, where                              # (the ABI call returns the size)
                    got = gx.containment(gy)
                    assert (got == cont) if x.size else (got != got), where
                    calls += 5
        launched = _launches(pkg, "compare_pair")
    finally:
        L.smh_profile_enable(0)
    assert launched == calls and calls > 0, (launched, calls)


# ---------------------------------------------------------------------------------------------- wave route
# wave_compare_pair cuts the merged sequence into 64 shares of ceil((la + lb) / 64): 129 and 192 give an odd share (3).
@pytest.mark.parametrize("total", [0, 1, 63, 64, 65, 129, 192, 257, 1025])
def test_wave_route_on_every_structure(total, pkg):
    """Rows: every structure's a once per cut position, that num on the row (smh_compare_block: per-row nums); columns: every
    structure's b.  Then the same sketches as a device CSR with one num per launch (smh_compare_block_dev)."""
    rng = np.random.default_rng(2000 + total)
    st = PR.structures(total, rng)
    share = -(-total // 64)
    rows, nums = [], []
    for name, a, b in st:
        for n in _cuts(a, b, share):
            rows.append(a); nums.append(n)
    cols = [b for _, _, b in st]
    grow = [_mh(pkg, a, n) for a, n in zip(rows, nums)]
    gcol = [_mh(pkg, b, 9) for b in cols]
    exp = PR.matrix(rows, cols, nums)
    out = _block(pkg, "wave", lambda: pkg.matrix.compare_block(grow, gcol, want=ALL))
    _same(out, exp, ALL, ("per-row nums", total))
    auto = _block(pkg, "auto", lambda: pkg.matrix.compare_block(grow, gcol, want=ALL))
    for k in ALL:
        assert np.array_equal(out[k], auto[k], equal_nan=True), k
    if total < 2:
        return                                   # (no hash on one of the sides: nothing to put into a device CSR)
    arows = [a for _, a, _ in st]
    rt, ro = _dev(pkg, arows)
    ct, co = _dev(pkg, cols)
    for n in sorted(set(_cuts(st[0][1], st[0][2], share) + _cuts(st[-3][1], st[-3][2], share))):
        exp = PR.matrix(arows, cols, n)
        out = _block(pkg, "wave", lambda: pkg.matrix.compare_block_dev(rt, ro, ct, co, n, want=ALL))
        _same(out, exp, ALL, ("one num", total, n))
        auto = _block(pkg, "auto", lambda: pkg.matrix.compare_block_dev(rt, ro, ct, co, n, want=ALL))
        for k in ALL:
            assert np.array_equal(_np(out[k]), _np(auto[k]), equal_nan=True), (k, n)


def _ragged_short(rng, count, lens, pool):
    return [np.sort(rng.choice(pool, lens[int(rng.integers(0, len(lens)))], replace=False)) for _ in range(count)]


def test_wave_route_workgroups_take_a_second_pair(pkg):
    """More pairs than the 32 * cu_count workgroups of k_compare_wave<true>: every workgroup restages A and B of its next
    pair into the LDS the previous pair used.  Short ragged sketches with empties among them, lengths drawn at random, so
    that the pairs a workgroup takes one after the other (pair ids gridDim.x apart) differ in length both ways."""
    rng = np.random.default_rng(2100)
    grid = 32 * _cu_count(pkg)
    ncols = 97
    nrows = grid // ncols + 9                                       # 8 rows' worth of pairs beyond the grid
    assert nrows * ncols > grid + ncols
    pool = np.unique(np.concatenate([PR.EXTREMES, rng.integers(1, (1 << 64) - 2, size=150, dtype=U64)]))
    lens = [0, 0, 1, 2, 3, 5, 8, 13, 31, 64, 65, 100]
    rows, cols = _ragged_short(rng, nrows, lens, pool), _ragged_short(rng, ncols, lens, pool)
    la = np.array([len(r) for r in rows])[:, None] + np.array([len(c) for c in cols])[None, :]
    flat = la.reshape(-1)
    nxt = flat[grid:] - flat[:flat.size - grid]                     # a workgroup's second pair against its first
    assert (nxt > 0).any() and (nxt < 0).any() and (flat[grid:] == 0).any()
    cuts = [0, 1, 2, 3, 7, 30, 64, 65, 150]
    nums = [cuts[i % len(cuts)] for i in range(nrows)]
    grow = [_mh(pkg, r, n) for r, n in zip(rows, nums)]
    gcol = [_mh(pkg, c, 9) for c in cols]
    out = _block(pkg, "wave", lambda: pkg.matrix.compare_block(grow, gcol, want=ALL))
    _same(out, PR.matrix(rows, cols, nums), ALL, "per-row nums")
    auto = _block(pkg, "auto", lambda: pkg.matrix.compare_block(grow, gcol, want=ALL))
    for k in ALL:
        assert np.array_equal(out[k], auto[k], equal_nan=True), k
    rt, ro = _dev(pkg, rows)
    ct, co = _dev(pkg, cols)
    out = _block(pkg, "wave", lambda: pkg.matrix.compare_block_dev(rt, ro, ct, co, 30, want=ALL))
    _same(out, PR.matrix(rows, cols, 30), ALL, "one num")
    auto = _block(pkg, "auto", lambda: pkg.matrix.compare_block_dev(rt, ro, ct, co, 30, want=ALL))
    for k in ALL:
        assert np.array_equal(_np(out[k]), _np(auto[k]), equal_nan=True), k


@pytest.mark.parametrize("total", [8192, 8193])
def test_wave_route_at_the_lds_switch(total, pkg):
    """Three by three with max_row_len + max_col_len == total: 8192 is the last size staged in LDS (k_compare_wave<true>,
    64 KiB), 8193 the first walked in global memory (k_compare_wave<false>).  Per-row nums from the cut positions."""
    rng = np.random.default_rng(2200 + total)
    st = {name: (a, b) for name, a, b in PR.structures(total, rng)}
    picked = [st["identical-both"], st["half-overlap-one"], st["a-below-b-one"]]
    rows = [a for a, _ in picked]
    cols = [b for _, b in picked]
    assert max(map(len, rows)) + max(map(len, cols)) == total
    share = -(-total // 64)
    cuts = [_cuts(a, b, share) for a, b in picked]
    ct, co = _dev(pkg, cols)
    rt, ro = _dev(pkg, rows)
    gcol = [_mh(pkg, b, 9) for b in cols]
    for k in range(max(map(len, cuts))):
        nums = [c[k % len(c)] for c in cuts]
        grow = [_mh(pkg, a, n) for a, n in zip(rows, nums)]
        out = _block(pkg, "wave", lambda: pkg.matrix.compare_block(grow, gcol, want=ALL))
        _same(out, PR.matrix(rows, cols, nums), ALL, nums)
        auto = _block(pkg, "auto", lambda: pkg.matrix.compare_block(grow, gcol, want=ALL))
        for name in ALL:
            assert np.array_equal(out[name], auto[name], equal_nan=True), (name, nums)
        out = _block(pkg, "wave", lambda: pkg.matrix.compare_block_dev(rt, ro, ct, co, nums[0], want=ALL))
        _same(out, PR.matrix(rows, cols, nums[0]), ALL, nums[0])


# ---------------------------------------------------------------------------------------------- few route
# launch_compare_block: the side with more sketches (rows on a tie) is streamed ("many"), the other sits in LDS while its
# longest sketch holds at most 8192 hashes (QLds); count_common or containment asked for selects WantCC.
def _few_block(pkg, rows, cols, nums, where):
    """compare_block on the few route, all five outputs and jaccard / common / size alone; both against the restatement"""
    grow = [_mh(pkg, r, n) for r, n in zip(rows, nums)]
    gcol = [_mh(pkg, c, 9) for c in cols]
    exp = PR.matrix(rows, cols, nums)
    out = _block(pkg, "few", lambda: pkg.matrix.compare_block(grow, gcol, want=ALL))
    _same(out, exp, ALL, where)
    out3 = _block(pkg, "few", lambda: pkg.matrix.compare_block(grow, gcol, want=NO_CC))
    _same(out3, exp, NO_CC, where)
    for k in NO_CC:
        assert np.array_equal(out3[k], out[k]), (where, k)
    return out


MANY_LENS = [0, 1, 63, 64, 65, 127, 128, 129, 1000]


@pytest.mark.parametrize("qmax", [8192, 8193])
@pytest.mark.parametrize("many_is_row", [1, 0])
def test_few_route_lengths(many_is_row, qmax, pkg):
    """Streamed sketches of every length around the 64-element steps against queries of 0, 1, 100 and qmax hashes: 8192 is
    the longest query kept in LDS, 8193 is searched in global memory.  Per length: a random draw from the pool the queries
    come from, a piece of the long query (every element matches), and hashes below / above all of the query's."""
    rng = np.random.default_rng(3000 + qmax)
    pool = _pool(rng, 12000)
    q_long = np.sort(rng.choice(pool, qmax, replace=False))
    few = [np.zeros(0, dtype=U64), q_long[4000:4001].copy(), np.sort(rng.choice(q_long, 100, replace=False)), q_long]
    many = []
    for k in MANY_LENS:
        start = int(rng.integers(0, qmax - k))
        many += [np.sort(rng.choice(pool, k, replace=False)), q_long[start:start + k].copy(),
                 np.arange(1, k + 1, dtype=U64) if k % 2 else (U64((1 << 64) - 2) - np.arange(k, dtype=U64))[::-1].copy()]
    many.append(PR.EXTREMES.copy())
    cuts = [0, 1, 5, 63, 64, 65, 128, 129, 1000, 5000, qmax, qmax + 1]
    rows, cols = (many, few) if many_is_row else (few, many)
    assert len(many) > len(few)
    if many_is_row:
        nums = [cuts[i % len(cuts)] for i in range(len(rows))]
        _few_block(pkg, rows, cols, nums, "many on the rows")
    else:
        for shift in range(0, len(cuts), 4):                      # the few rows take every cut in three launches
            nums = [cuts[(shift + i) % len(cuts)] for i in range(len(rows))]
            _few_block(pkg, rows, cols, nums, ("few on the rows", shift))
    # the same lengths as a device CSR, one num
    rt, ro = _dev(pkg, rows)
    ct, co = _dev(pkg, cols)
    for n in (0, 64, 1000):
        exp = PR.matrix(rows, cols, n)
        for want in (ALL, NO_CC):
            out = _block(pkg, "few", lambda: pkg.matrix.compare_block_dev(rt, ro, ct, co, n, want=want))
            _same(out, exp, want, ("one num", n))


def _pool(rng, k):
    return np.unique(np.concatenate([PR.EXTREMES, rng.integers(1, (1 << 64) - 2, size=k, dtype=U64)]))


def _exit_nums(a, q):
    """wave_pair streams `a` 64 elements a step.  For every FULL step: the union rank u (from 0) of the step's last element
    -- lane 63's -- and the nums that make it n - 2, n - 1, n and n + 1; the early exit is taken from u >= n on (at n - 2 the
    next element still counts when it matches: an exit taken there would lose it)."""
    u = np.union1d(a, q)
    ns = set()
    for last in range(63, a.size, 64):
        r = int(np.searchsorted(u, a[last]))
        ns.update([r - 1, r, r + 1, r + 2])
    return sorted(n for n in ns if n >= 1)


@pytest.mark.parametrize("many_is_row", [1, 0])
def test_few_route_early_exit_edges(many_is_row, pkg):
    """Streamed lengths 64 and 128 (the last full step is the final one), 65 and 129 (a ragged step follows it) against
    queries that overlap, equal (ragged tail included), interleave with, lie below, lie above and miss the streamed sketch,
    with the num that puts lane 63's union rank at n - 2, n - 1, n and n + 1 on every full step.  The exit exists in the
    WantCC = false instantiation only; both are run and must agree."""
    rng = np.random.default_rng(3100)
    pool = _pool(rng, 400)
    streamed = [np.sort(rng.choice(pool, k, replace=False)) for k in (64, 128, 65, 129)]
    lo = np.arange(1, 41, dtype=U64)
    queries = [np.sort(rng.choice(pool, 150, replace=False)), streamed[1].copy(), streamed[3][1::2].copy(), lo,
               (U64((1 << 64) - 2) - lo)[::-1].copy(), np.zeros(0, dtype=U64), streamed[3][:64].copy(), streamed[2].copy(),
               streamed[3].copy()]
    fill = [np.sort(rng.choice(pool, k, replace=False)) for k in (0, 1, 63, 200, 7, 30)]
    if many_is_row:
        rows, nums = [], []
        for a in streamed:
            for q in queries:
                for n in _exit_nums(a, q):
                    rows.append(a); nums.append(n)
        assert len(rows) > 100
        _few_block(pkg, rows, queries, nums, "many on the rows")
    else:
        cols = streamed + fill + fill                              # more columns than rows: the columns are streamed
        for q in queries:
            for a in streamed:
                nums = _exit_nums(a, q)
                assert 4 <= len(nums) <= 8 and len(nums) < len(cols)
                _few_block(pkg, [q] * len(nums), cols, nums, ("few on the rows", q.size, a.size))


@pytest.mark.parametrize("n_many", [1, 3, 4, 5, 63, 64, -1])
def test_few_route_counts_of_streamed_sketches(n_many, pkg):
    """A workgroup's four waves take four streamed sketches: counts around that, around a wave's worth of them, and (-1) more
    than the 4 * 8 * cu_count the grid covers in one pass, so that the grid-stride loop runs.  Tiny ragged sketches, both
    orientations (one streamed sketch can only be a row: rows are streamed on a tie)."""
    rng = np.random.default_rng(3200 + n_many)
    if n_many < 0:
        n_many = 4 * 8 * _cu_count(pkg) + 37
    pool = _pool(rng, 60)
    if n_many == 1:
        # one against one: smh_compare_block would serve it on the pair path, the device CSR call goes by the pinned route
        a, q = np.sort(rng.choice(pool, 6, replace=False)), np.sort(rng.choice(pool, 40, replace=False))
        rt, ro = _dev(pkg, [a])
        ct, co = _dev(pkg, [q])
        for n in (0, 1, 5, 41, 44):
            for want in (ALL, NO_CC):
                out = _block(pkg, "few", lambda: pkg.matrix.compare_block_dev(rt, ro, ct, co, n, want=want))
                _same(out, PR.matrix([a], [q], n), want, n)
        return
    many = _ragged_short(rng, n_many, [0, 1, 2, 3, 4, 6], pool)
    few = [np.sort(rng.choice(pool, k, replace=False)) for k in (40, 5)][:max(1, min(2, n_many - 1))]
    cuts = [0, 1, 2, 3, 5, 41, 44]
    out = _few_block(pkg, many, few, [cuts[i % len(cuts)] for i in range(n_many)], "many on the rows")
    assert out["size"].shape == (n_many, len(few))
    if n_many > len(few):
        _few_block(pkg, few, many, [3, 42][:len(few)], "few on the rows")
        _few_block(pkg, few, many, [0, 5][:len(few)], "few on the rows")


@pytest.mark.parametrize("route", ["wave", "few"])
def test_resident_index_find_on_the_small_routes(route, pkg):
    """ResidentIndex.find: node i is a hit when node_i.compare(query) -- cut by the NODE's num -- or node_i.containment(query)
    exceeds the threshold (an empty node's containment is NaN: never a hit)."""
    rng = np.random.default_rng(3300)
    st = PR.structures(129, rng) + PR.structures(64, rng)[:4]
    nodes, nums = [], []
    for i, (name, a, b) in enumerate(st):
        for s, n in ((a, _cuts(a, b, 3)[i % 5 + 1]), (b, 0)):
            nodes.append(s); nums.append(n)
    gnodes = [_mh(pkg, s, n) for s, n in zip(nodes, nums)]
    idx = pkg.index.ResidentIndex(gnodes)
    for q in (st[0][2], st[9][1], st[2][1][::3].copy(), np.zeros(0, dtype=U64)):
        gq = _mh(pkg, q, 50)
        exp = PR.matrix(nodes, [q], nums)
        for thr in (0.0, 0.05, 0.3, 0.5, 0.999):
            hits = _block(pkg, route, lambda: idx.find(gq, thr))
            assert hits == [i for i in range(len(nodes)) if exp["jaccard"][i, 0] > thr], (route, q.size, thr)
            hits = _block(pkg, route, lambda: idx.find(gq, thr, containment=True))
            assert hits == [i for i in range(len(nodes)) if exp["containment"][i, 0] > thr], (route, q.size, thr)
