"""Downsampling on the device against tests/downsample_restatement.py: the block call at the sizes where
the copy kernel's code changes (T = output elements per workgroup and the wave, both from smh_downsample_geometry), the cut
of a sketch that lives in HBM, the cut of a resident index, the downsample=True routes, and the wide-abundance rule."""
import ctypes as C

import numpy as np
import pytest

import downsample_restatement as R

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
MX = 1 << 62           # the max_hash most block cases cut at


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


@pytest.fixture(scope="module")
def T(pkg):
    tile, threads = pkg.matrix.downsample_geometry()
    assert tile >= 256 and threads % 64 == 0 and tile % threads == 0
    return tile


# ---------------------------------------------------------------------------------- the block call

def seg(rng, keep, drop, mx=MX):
    """an ascending sketch with `keep` hashes <= mx and `drop` hashes above it"""
    lo = np.uint64(10) + np.cumsum(rng.integers(1, 1000, keep, dtype=np.uint64), dtype=np.uint64)
    hi = np.uint64(mx) + np.cumsum(rng.integers(1, 1000, drop, dtype=np.uint64), dtype=np.uint64)
    return np.concatenate([lo, hi]).astype(np.uint64)


def position_abunds(n, base=0):
    """abundances that name the position they stand at: a copy shifted by one element shows"""
    return ((np.arange(base, base + n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def run_block(pkg, segs, mx, with_abunds, lead=0):
    """the library's cut of the CSR of `segs` and the restatement's; lead: junk elements in front (offsets[0] = lead)"""
    import torch
    flat = np.concatenate([np.zeros(lead, np.uint64)] + [np.asarray(s, np.uint64) for s in segs]) if (segs or lead) else np.zeros(0, np.uint64)
    off = np.zeros(len(segs) + 1, dtype=np.uint64)
    off[0] = lead
    for i, s in enumerate(segs):
        off[i + 1] = off[i] + np.uint64(len(s))
    ab = position_abunds(flat.size) if with_abunds else None
    d_flat = torch.from_numpy(np.concatenate([flat, np.zeros(1, np.uint64)]).view(np.int64)).cuda()
    d_ab = torch.from_numpy(np.concatenate([ab, np.zeros(1, np.uint32)]).view(np.int32)).cuda() if with_abunds else None
    out_h, out_a, new_off = pkg.matrix.downsample_block_dev(d_flat, off, mx, abunds=d_ab)
    want_h, want_a, want_off = R.cut_csr(flat, ab, off, mx)
    total = int(new_off[-1])
    assert new_off.tolist() == want_off.tolist()
    got_h = out_h.cpu().numpy().view(np.uint64)[:total]
    assert np.array_equal(got_h, want_h)
    if with_abunds:
        assert np.array_equal(out_a.cpu().numpy().view(np.uint32)[:total], want_a)
    else:
        assert out_a is None
    return np.diff(new_off.astype(np.int64)).tolist()


both = pytest.mark.parametrize("with_abunds", [False, True], ids=["hashes", "abunds"])


@both
def test_block_empty_collections(pkg, with_abunds):
    assert run_block(pkg, [], MX, with_abunds) == []
    assert run_block(pkg, [np.zeros(0, np.uint64)], MX, with_abunds) == [0]
    assert run_block(pkg, [np.zeros(0, np.uint64)] * 5, MX, with_abunds) == [0] * 5


@both
def test_block_all_none_and_the_inclusive_bound(pkg, with_abunds):
    rng = np.random.default_rng(1)
    segs = [seg(rng, k, d) for k, d in ((10, 3), (0, 4), (200, 0), (1, 1), (0, 0), (77, 77))]
    assert run_block(pkg, segs, M64, with_abunds) == [len(s) for s in segs]
    smallest = min(int(s[0]) for s in segs if len(s))
    assert smallest > 0 and run_block(pkg, segs, smallest - 1, with_abunds) == [0] * len(segs)
    # max_hash equal to an element keeps it, one less drops it
    e = int(segs[2][100])
    assert run_block(pkg, segs, e, with_abunds)[2] == 101
    assert run_block(pkg, segs, e - 1, with_abunds)[2] == 100


@both
def test_block_compares_unsigned(pkg, with_abunds):
    half = 1 << 63
    a = np.array([5, half - 2, half - 1, half, half + 1, M64 - 1, M64], dtype=np.uint64)
    b = np.array([half + 7, half + 9], dtype=np.uint64)
    c = np.array([1, 2, 3], dtype=np.uint64)
    assert run_block(pkg, [a, b, c], half, with_abunds) == [4, 0, 3]
    assert run_block(pkg, [a, b, c], half + 8, with_abunds) == [5, 1, 3]
    assert run_block(pkg, [a, b, c], M64 - 1, with_abunds) == [6, 2, 3]
    assert run_block(pkg, [a, b, c], half - 1, with_abunds) == [3, 0, 3]


@both
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_block_segment_ends_around_tile_ends(pkg, T, with_abunds, descending):
    rng = np.random.default_rng(2)
    keeps = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    if descending:
        keeps = keeps[::-1]
    segs = [seg(rng, k, int(rng.integers(0, 70))) for k in keeps]
    assert run_block(pkg, segs, MX, with_abunds) == keeps


@both
def test_block_long_stretch_that_keeps_nothing(pkg, T, with_abunds):
    rng = np.random.default_rng(3)
    segs = [seg(rng, 100, 5)] + [seg(rng, 0, int(rng.integers(0, 3))) for _ in range(T + 7)] + [seg(rng, T + 100, 9)]
    assert run_block(pkg, segs, MX, with_abunds) == [100] + [0] * (T + 7) + [T + 100]


@both
def test_block_one_long_sketch_among_tiny_ones(pkg, T, with_abunds):
    rng = np.random.default_rng(4)
    tiny = lambda k: [seg(rng, int(x), int(rng.integers(0, 4))) for x in rng.integers(0, 6, k)]
    segs = tiny(300) + [seg(rng, 5 * T + 3, 11)] + tiny(300)
    got = run_block(pkg, segs, MX, with_abunds)
    assert got[300] == 5 * T + 3


@both
@pytest.mark.parametrize("per_sketch", [3, 4, 5])
def test_block_many_tiny_sketches_per_tile(pkg, T, with_abunds, per_sketch):
    """a tile of T outputs then crosses about T / per_sketch segments: around, above and below what the kernel stages in LDS"""
    rng = np.random.default_rng(5)
    n = 2 * T // per_sketch + 50
    segs = [seg(rng, per_sketch, int(rng.integers(0, 3))) for _ in range(n)]
    assert run_block(pkg, segs, MX, with_abunds) == [per_sketch] * n


@both
@pytest.mark.parametrize("lead", [0, 1, 3])
def test_block_source_parity_against_destination(pkg, T, with_abunds, lead):
    """dropped tails of odd and even length in front of a long sketch: its source starts at either 16-byte parity, and at
    every position of a group of four, while its destination does not move"""
    rng = np.random.default_rng(6)
    for drop in (0, 1, 2, 3, 4, 7):
        segs = [seg(rng, 8, drop), seg(rng, T + 37, 2), seg(rng, 3, 1), seg(rng, 2 * T, 0)]
        assert run_block(pkg, segs, MX, with_abunds, lead=lead) == [8, T + 37, 3, 2 * T]


@both
def test_block_outputs_off_the_16_byte_grid(pkg, T, with_abunds):
    """output tensors that begin one element into an allocation: the copy then stores element by element"""
    import torch
    rng = np.random.default_rng(9)
    segs = [seg(rng, 70, 3), seg(rng, 0, 2), seg(rng, T + 5, 1)]
    flat = np.concatenate(segs)
    off = np.array([0, 73, 75, 75 + T + 6], dtype=np.uint64)
    ab = position_abunds(flat.size)
    d_flat = torch.from_numpy(flat.view(np.int64)).cuda()
    d_ab = torch.from_numpy(ab.view(np.int32)).cuda() if with_abunds else None
    out_h = torch.full((T + 77,), -7, dtype=torch.int64, device="cuda")
    out_a = torch.full((T + 77,), -9, dtype=torch.int32, device="cuda") if with_abunds else None
    _, _, new_off = pkg.matrix.downsample_block_dev(d_flat, off, MX, abunds=d_ab, out_hashes=out_h[1:-1],
                                                    out_abunds=out_a[1:-1] if with_abunds else None)
    want_h, want_a, want_off = R.cut_csr(flat, ab if with_abunds else None, off, MX)
    assert new_off.tolist() == want_off.tolist() == [0, 70, 70, T + 75]
    got = out_h.cpu().numpy()
    assert got[0] == -7 and got[-1] == -7 and np.array_equal(got[1:-1].view(np.uint64), want_h)
    if with_abunds:
        got = out_a.cpu().numpy()
        assert got[0] == -9 and got[-1] == -9 and np.array_equal(got[1:-1].view(np.uint32), want_a)


@both
def test_block_capacity_one_short_writes_nothing(pkg, T, with_abunds):
    import torch
    rng = np.random.default_rng(7)
    segs = [seg(rng, 50, 5), seg(rng, T, 3)]
    flat = np.concatenate(segs)
    off = np.array([0, 55, 55 + T + 3], dtype=np.uint64)
    d_flat = torch.from_numpy(flat.view(np.int64)).cuda()
    d_ab = torch.from_numpy(position_abunds(flat.size).view(np.int32)).cuda() if with_abunds else None
    out_h = torch.full((T + 49,), -7, dtype=torch.int64, device="cuda")
    out_a = torch.full((T + 49,), -9, dtype=torch.int32, device="cuda") if with_abunds else None
    with pytest.raises(pkg.SourmashError) as ei:
        pkg.matrix.downsample_block_dev(d_flat, off, MX, abunds=d_ab, out_hashes=out_h, out_abunds=out_a)
    assert ei.value.code == 3 and str(T + 50) in ei.value.message and str(T + 49) in ei.value.message
    assert bool((out_h == -7).all()) and (out_a is None or bool((out_a == -9).all()))
    # with room for it the same call fills exactly the kept total
    out_h = torch.full((T + 50,), -7, dtype=torch.int64, device="cuda")
    out_a = torch.full((T + 50,), -9, dtype=torch.int32, device="cuda") if with_abunds else None
    _, _, new_off = pkg.matrix.downsample_block_dev(d_flat, off, MX, abunds=d_ab, out_hashes=out_h, out_abunds=out_a)
    assert new_off.tolist() == [0, 50, T + 50]
    assert np.array_equal(out_h.cpu().numpy().view(np.uint64), R.cut_csr(flat, None, off, MX)[0])


def test_block_timers_and_refusals(pkg):
    import torch
    L = pkg.lib()
    d = torch.from_numpy(np.arange(1, 11, dtype=np.int64)).cuda()
    L.smh_profile_enable(1)
    try:
        L.smh_profile_reset()
        pkg.matrix.downsample_block_dev(d, [0, 4, 10], 7)
        assert count(pkg, "downsample_bounds") == 1 and count(pkg, "downsample_copy") == 1
    finally:
        L.smh_profile_enable(0)
    with pytest.raises(pkg.SourmashError) as ei:
        pkg.matrix.downsample_block_dev(d, [0, 4, 10], 0)
    assert ei.value.code == 3
    with pytest.raises(pkg.SourmashError) as ei:
        pkg.matrix.downsample_block_dev(d, [0, 6, 4], 7)
    assert ei.value.code == 3


# ---------------------------------------------------------------------------------- a sketch that lives in HBM

@pytest.mark.parametrize("track", [False, True], ids=["flat", "tracked"])
@pytest.mark.parametrize("batches", [1, 2], ids=["run-starts", "counts"])
def test_device_sketch_cut(pkg, coracle, track, batches):
    from sourmash_rust_amd.index import max_hash_of_scaled
    fine, coarse = max_hash_of_scaled(10), max_hash_of_scaled(100)
    parts = [bytes(coracle.synth_dna(0, 20000, 11, 0)), bytes(coracle.synth_dna(5000, 20000, 11, 0))][:batches]

    def sketch(mx):
        mh = pkg.KmerMinHash(0, 21, False, 42, mx, track)
        for p in parts:
            mh.add_sequences([p], True)
        return mh

    twin = sketch(fine)
    mins, abunds = twin.mins, twin.abunds          # (the twin comes to the host; the sketches cut below do not)
    assert len(mins) > 1500 and (not track or max(abunds) > 1 or batches == 1)
    ref = sketch(coarse)
    cuts = {"scaled=100": coarse, "everything": fine, "nothing": mins[0] - 1, "on the last hash": mins[-1],
            "below the last hash": mins[-1] - 1}
    for what, mx in cuts.items():
        src = sketch(fine)
        before = count(pkg, "sketch_to_host")
        got = src.downsample_max_hash(mx)
        assert count(pkg, "sketch_to_host") == before, "the cut brought a sketch to the host (%s)" % what
        want_m, want_a = R.cut(mins, abunds, mx)
        assert len(got) == len(want_m) and got.max_hash == mx and got.track_abundance == track and got.ksize == 21
        assert count(pkg, "sketch_to_host") == before
        assert got.mins == want_m and got.abunds == want_a, what
        if want_m:   # the result lived in HBM: looking at it moved it
            assert count(pkg, "sketch_to_host") == before + 1
        assert src.mins == mins and src.abunds == abunds, "the source changed (%s)" % what
        assert count(pkg, "sketch_to_host") == before + 1 + bool(want_m)
        if what == "scaled=100":
            assert got.mins == ref.mins and got.abunds == ref.abunds and len(want_m) > 100
    # a cut sketch goes on accumulating like any other
    src = sketch(fine)
    got = src.downsample_max_hash(coarse)
    more = bytes(coracle.synth_dna(40000, 20000, 11, 0))
    got.add_sequences([more], True)
    ref.add_sequences([more], True)
    assert got.mins == ref.mins and got.abunds == ref.abunds


# ---------------------------------------------------------------------------------- the index

def mk(pkg, mins, abunds, max_hash, num=0, ksize=21, seed=42, protein=False):
    mh = pkg.KmerMinHash(num, ksize, protein, seed, max_hash, abunds is not None)
    if abunds is not None:
        mh.add_many_with_abund(list(zip(mins, abunds)))
    elif len(mins):
        mh.add_many(np.array(mins, dtype=np.uint64))
    return mh


FIVE = ("jaccard", "common", "size", "count_common", "containment")


def same_matrices(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)), k


def same_index(pkg, cut, rebuilt, queries, angular=True):
    """everything the index serves, on the device cut and on an index rebuilt from sketches cut on the host"""
    assert len(cut) == len(rebuilt) and cut.max_hash_range == rebuilt.max_hash_range
    same_matrices(cut.compare(cut, want=FIVE), rebuilt.compare(rebuilt, want=FIVE))
    same_matrices(cut.compare(rebuilt, want=FIVE), rebuilt.compare(rebuilt, want=FIVE))
    for q in queries:
        for cont in (False, True):
            assert cut.find(q, 0.01, cont) == rebuilt.find(q, 0.01, cont)
        assert cut.most_common(q) == rebuilt.most_common(q)
        g, e = cut.gather(q, threshold_bp=0), rebuilt.gather(q, threshold_bp=0)
        assert g.rows == e.rows and len(e.rows) > 0 and np.array_equal(g.assigned, e.assigned)
    assert cut.has_abundances == rebuilt.has_abundances
    if angular and cut.has_abundances:
        assert cut.norms2().tolist() == rebuilt.norms2().tolist()
        want = ("dot", "cosine", "angular")
        same_matrices(cut.angular_matrix(want=want), rebuilt.angular_matrix(want=want))
        for q in queries:
            for x, y in zip(cut.angular(q), rebuilt.angular(q)):
                assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


class Fixture:
    """the 100 sketches of the committed fixture (scaled, with abundances) at their own max_hash and cut to a quarter"""
    def __init__(self, pkg, sketches):
        self.fine_mx = sketches[0]["max_hash"]
        self.coarse_mx = self.fine_mx // 4
        self.S = [(s["mins"], s["abundances"]) for s in sketches]
        self.C = [R.cut(m, a, self.coarse_mx) for m, a in self.S]
        assert sum(len(m) for m, _ in self.C) > 30000
        self.fine_nodes = [mk(pkg, m, a, self.fine_mx) for m, a in self.S]
        self.coarse_nodes = [mk(pkg, m, a, self.coarse_mx) for m, a in self.C]
        self.fine = pkg.index.ResidentIndex(self.fine_nodes)
        self.coarse = pkg.index.ResidentIndex(self.coarse_nodes)
        self.coarse_twin = pkg.index.ResidentIndex(self.coarse_nodes)   # (an index against ITSELF sets the angular diagonal)


@pytest.fixture(scope="module")
def fx(pkg, sbt_subset_sketches):
    return Fixture(pkg, sbt_subset_sketches)


def test_index_cut_of_the_fixture(pkg, fx):
    before = count(pkg, "index_downsampled")
    cut = fx.fine.downsample(max_hash=fx.coarse_mx)
    assert count(pkg, "index_downsampled") == before + 1
    assert fx.fine.max_hash == fx.fine_mx and cut.max_hash == fx.coarse_mx and cut.max_hash_range == (fx.coarse_mx, fx.coarse_mx)
    assert fx.fine.downsample(max_hash=fx.coarse_mx) is cut and count(pkg, "index_downsampled") == before + 1
    same_index(pkg, cut, fx.coarse, [fx.coarse_nodes[0], fx.coarse_nodes[57]])
    # through scaled=, and at the index's own resolution (an equal copy)
    from sourmash_rust_amd.index import max_hash_of_scaled, scaled_of_max_hash
    s = scaled_of_max_hash(fx.fine_mx) * 3
    by_scaled = fx.fine.downsample(scaled=s)
    assert by_scaled.max_hash == max_hash_of_scaled(s)
    rebuilt = pkg.index.ResidentIndex([mk(pkg, *R.cut(m, a, max_hash_of_scaled(s)), max_hash_of_scaled(s)) for m, a in fx.S])
    same_index(pkg, by_scaled, rebuilt, [rebuilt.nodes[3]], angular=False)
    same_index(pkg, fx.fine.downsample(max_hash=fx.fine_mx), fx.fine, [fx.fine_nodes[3]], angular=False)
    fx.fine.drop_downsampled()


def test_index_cut_after_the_abundances_moved_to_hbm(pkg, fx):
    """an index that has served an angular call holds its abundances in HBM: the copy kernel cuts them, also for a cut of a cut"""
    parent = pkg.index.ResidentIndex(fx.fine_nodes)
    parent.norms2()
    half = fx.fine_mx // 2
    mid = parent.downsample(max_hash=half)
    rebuilt = pkg.index.ResidentIndex([mk(pkg, *R.cut(m, a, half), half) for m, a in fx.S])
    assert mid.norms2().tolist() == rebuilt.norms2().tolist()
    fresh = parent.downsample(max_hash=fx.coarse_mx)
    grandchild = pkg.index.ResidentIndex(fx.fine_nodes).downsample(max_hash=half)   # abundances still on the host here
    for cut in (fresh, mid.downsample(max_hash=fx.coarse_mx), grandchild.downsample(max_hash=fx.coarse_mx)):
        same_index(pkg, cut, fx.coarse, [fx.coarse_nodes[9]])


def family(rng, pool, n, k):
    out = []
    for _ in range(n):
        idx = np.sort(rng.choice(len(pool), k, replace=False))
        out.append(([int(pool[i]) for i in idx], [int(x) for x in rng.integers(1, 50, k)]))
    return out


def test_index_cut_of_small_families_and_mixed_resolutions(pkg):
    rng = np.random.default_rng(8)
    top = 1 << 60
    pool = np.unique(rng.integers(1, top, 3000, dtype=np.uint64))
    fam = family(rng, pool, 12, 400) + [([], [])] + family(rng, pool, 3, 5)
    mxs = [top, top // 2, top // 3, top]        # the nodes' own resolutions, in turn
    nodes = [mk(pkg, *R.cut(m, a, mxs[i % 4]), mxs[i % 4]) for i, (m, a) in enumerate(fam)]
    mixed = pkg.index.ResidentIndex(nodes)
    assert mixed.max_hash is None and mixed.max_hash_range == (top // 3, top)
    with pytest.raises(pkg.SourmashError) as ei:
        mixed.compare(mixed)
    assert ei.value.code == 103
    for target in (top // 3, top // 7):
        rebuilt = pkg.index.ResidentIndex([mk(pkg, *R.cut(m, a, target), target) for m, a in fam])
        q = rebuilt.nodes[1]
        same_index(pkg, mixed.downsample(max_hash=target), rebuilt, [q])
        same_index(pkg, pkg.index.ResidentIndex(nodes, max_hash=target), rebuilt, [q])
    same_matrices(mixed.compare(mixed, want=FIVE, downsample=True),
                  pkg.index.ResidentIndex(nodes, max_hash=top // 3).compare(mixed.downsample(max_hash=top // 3), want=FIVE))
    for bad in (0, top // 3 + 1, top):
        with pytest.raises(pkg.SourmashError) as ei:
            mixed.downsample(max_hash=bad)
        assert ei.value.code == 3
    # the constructor form reports the same refusals, and the process goes on working after each
    num_nodes = nodes[:2] + [mk(pkg, [1, 2, 3], [1, 1, 1], 0, num=5)]
    for bad_nodes, bad in ((num_nodes, 5), (nodes, top // 3 + 1), (nodes, top), (nodes, 0)):
        with pytest.raises(pkg.SourmashError) as ei:
            pkg.index.ResidentIndex(bad_nodes, max_hash=bad)
        assert ei.value.code == 3
        import gc
        gc.collect()      # the refused object is finalised here: it owns no handle
        again = pkg.index.ResidentIndex(nodes, max_hash=top // 3)
        same_matrices(again.compare(again, want=FIVE), mixed.downsample(max_hash=top // 3).compare(again, want=FIVE))
    with_num = pkg.index.ResidentIndex(num_nodes)
    with pytest.raises(pkg.SourmashError) as ei:
        with_num.downsample(max_hash=5)
    assert ei.value.code == 3 and "node 2" in ei.value.message
    empty = pkg.index.ResidentIndex([])
    assert empty.max_hash_range == (0, 0) and empty.max_hash is None and len(empty.downsample(max_hash=5)) == 0
    # untracked nodes: the child has no abundances either
    flat = pkg.index.ResidentIndex([mk(pkg, m, None, top) for m, _ in fam[:6]])
    child = flat.downsample(max_hash=top // 2)
    assert not child.has_abundances
    rebuilt = pkg.index.ResidentIndex([mk(pkg, R.cut(m, None, top // 2)[0], None, top // 2) for m, _ in fam[:6]])
    same_matrices(child.compare(child, want=FIVE), rebuilt.compare(rebuilt, want=FIVE))


# ---------------------------------------------------------------------------------- the downsample=True routes

def route_calls(want_index=False):
    """name -> call(index, operand); the operand is a sketch, or an index for compare"""
    def rows(res):
        return [tuple(r) for r in res.rows], res.assigned.tolist()
    return {
        "find": lambda idx, q, **kw: (idx.find(q, 0.02, **kw), idx.find(q, 0.02, True, **kw)),
        "most_common": lambda idx, q, **kw: idx.most_common(q, **kw),
        "gather": lambda idx, q, **kw: rows(idx.gather(q, threshold_bp=50000, **kw)),
        "angular": lambda idx, q, **kw: [x.view(np.uint64).tolist() for x in idx.angular(q, **kw)],
    }


@pytest.mark.parametrize("route", ["find", "most_common", "gather", "angular"])
def test_sketch_routes_meet_at_the_coarser_resolution(pkg, fx, route):
    call = route_calls()[route]
    fine_q, coarse_q = fx.fine_nodes[21], fx.coarse_nodes[21]
    # the query finer than the index
    with pytest.raises(pkg.SourmashError) as ei:
        call(fx.coarse, fine_q)
    assert ei.value.code == 103
    assert call(fx.coarse, fine_q, downsample=True) == call(fx.coarse, coarse_q)
    # the index finer than the query: its cut is made once and served from the cache after
    with pytest.raises(pkg.SourmashError) as ei:
        call(fx.fine, coarse_q)
    assert ei.value.code == 103
    fx.fine.drop_downsampled()
    before = count(pkg, "index_downsampled")
    expected = call(fx.coarse, coarse_q)
    assert call(fx.fine, coarse_q, downsample=True) == expected
    assert count(pkg, "index_downsampled") == before + 1
    assert call(fx.fine, coarse_q, downsample=True) == expected
    assert count(pkg, "index_downsampled") == before + 1
    fx.fine.drop_downsampled()
    assert call(fx.fine, coarse_q, downsample=True) == expected
    assert count(pkg, "index_downsampled") == before + 2
    # both equal: nothing is cut
    assert call(fx.fine, fine_q, downsample=True) == call(fx.fine, fine_q)
    assert count(pkg, "index_downsampled") == before + 2
    # a query that lives in HBM is cut there
    dev_q = mk(pkg, *fx.S[21], fx.fine_mx)
    assert dev_q.export_dev() == len(fx.S[21][0])
    assert call(fx.coarse, dev_q, downsample=True) == call(fx.coarse, coarse_q)
    to_host = count(pkg, "sketch_to_host")      # (find and most_common bring the CUT query to the host, as they do any query)
    assert dev_q.mins == fx.S[21][0] and count(pkg, "sketch_to_host") == to_host + 1, "the query itself had left HBM"


def test_gather_route_reports_the_cut_query(pkg, fx):
    from sourmash_rust_amd.index import scaled_of_max_hash
    fine_q, coarse_q = fx.fine_nodes[40], fx.coarse_nodes[40]
    res = fx.coarse.gather(fine_q, threshold_bp=0, downsample=True)
    exp = fx.coarse.gather(coarse_q, threshold_bp=0, scaled=scaled_of_max_hash(fx.coarse_mx))
    assert res.rows == exp.rows and np.array_equal(res.assigned, exp.assigned)
    assert res.assigned.size == len(coarse_q) < len(fine_q)
    assert res.rows[0].match == 40 and res.rows[0].f_orig_query == 1.0
    assert res.rows[0].remaining_bp == 0 * scaled_of_max_hash(fx.coarse_mx)


def test_compare_and_angular_matrix_routes(pkg, fx):
    for a, b, ea, eb in ((fx.fine, fx.coarse, fx.coarse, fx.coarse_twin), (fx.coarse, fx.fine, fx.coarse, fx.coarse_twin),
                         (fx.fine, fx.fine, fx.fine, fx.fine)):
        if a is not b:
            for fn in (lambda: a.compare(b), lambda: a.angular_matrix(b)):
                with pytest.raises(pkg.SourmashError) as ei:
                    fn()
                assert ei.value.code == 103
        fx.fine.drop_downsampled()
        before = count(pkg, "index_downsampled")
        same_matrices(a.compare(b, want=FIVE, downsample=True), ea.compare(eb, want=FIVE))
        moved = count(pkg, "index_downsampled") - before
        assert moved == (0 if a is b else 1)
        same_matrices(a.compare(b, want=FIVE, downsample=True), ea.compare(eb, want=FIVE))
        want = ("dot", "cosine", "angular")
        same_matrices(a.angular_matrix(b, want=want, downsample=True), ea.angular_matrix(eb, want=want))
        assert count(pkg, "index_downsampled") - before == moved
    fx.fine.drop_downsampled()


def test_routes_keep_the_other_refusals(pkg, fx):
    m, a = fx.S[5]
    cases = [(mk(pkg, m, a, fx.fine_mx, ksize=31), 101), (mk(pkg, m, a, fx.fine_mx, protein=True), 102),
             (mk(pkg, m, a, fx.fine_mx, seed=43), 104)]
    calls = route_calls()
    for q, code in cases:
        for name, call in calls.items():
            with pytest.raises(pkg.SourmashError) as ei:
                call(fx.coarse, q, downsample=True)
            assert ei.value.code == code, (name, code)
        other = pkg.index.ResidentIndex([q])
        for fn in (lambda: fx.coarse.compare(other, downsample=True), lambda: other.compare(fx.coarse, downsample=True),
                   lambda: fx.coarse.angular_matrix(other, downsample=True)):
            with pytest.raises(pkg.SourmashError) as ei:
                fn()
            assert ei.value.code == code
    num_q = mk(pkg, m[:50], a[:50], 0, num=50)
    for name, call in calls.items():
        with pytest.raises(pkg.SourmashError) as ei:
            call(fx.coarse, num_q, downsample=True)
        assert ei.value.code == 3, name
    num_index = pkg.index.ResidentIndex([num_q])
    for fn in (lambda: num_index.find(fx.coarse_nodes[0], 0.1, downsample=True), lambda: fx.coarse.compare(num_index, downsample=True),
               lambda: num_index.compare(fx.coarse, downsample=True), lambda: num_index.angular_matrix(downsample=True)):
        with pytest.raises(pkg.SourmashError) as ei:
            fn()
        assert ei.value.code == 3
    fx.fine.drop_downsampled()


# ---------------------------------------------------------------------------------- abundances of 2^32 or more

def test_wide_abundance_counts_only_where_the_cut_kept_it(pkg):
    top = 1 << 60
    plain = ([10, 20, 30, top - 5], [1, 2, 3, 4])
    wide_mins = [7, 20, 31, top - 9]

    def wide_node(mx):
        mh = pkg.KmerMinHash(0, 21, False, 42, mx, True)
        m, a = R.cut(wide_mins, [5, 6, 7, 1 << 32], mx)
        for h in m:
            mh.mins_push(h)
        for x in a:
            mh.abunds_push(x)
        return mh

    parent = pkg.index.ResidentIndex([mk(pkg, *plain, top), wide_node(top), mk(pkg, *plain, top)])
    assert parent.has_abundances

    def rebuilt(mx):
        return pkg.index.ResidentIndex([mk(pkg, *R.cut(*plain, mx), mx), wide_node(mx), mk(pkg, *R.cut(*plain, mx), mx)])

    dropped = parent.downsample(max_hash=1000)             # the wide abundance sits above the cut
    assert dropped.norms2().tolist() == rebuilt(1000).norms2().tolist() == [14, 110, 14]
    same_matrices(dropped.angular_matrix(want=("dot", "cosine")), rebuilt(1000).angular_matrix(want=("dot", "cosine")))
    assert dropped.angular(mk(pkg, [20], [3], 1000)).dot.tolist() == [6, 18, 6]
    kept = parent.downsample(max_hash=top - 9)             # ... and exactly on it
    for idx in (kept, rebuilt(top - 9), parent):
        for fn in (idx.norms2, idx.angular_matrix, lambda: idx.angular(mk(pkg, [20], [3], idx.max_hash))):
            with pytest.raises(pkg.SourmashError) as ei:
                fn()
            assert ei.value.code == 3 and "node 1" in ei.value.message
    # after the parent has tried (its abundances are in HBM now) the rule holds as well
    assert parent.downsample(max_hash=999).norms2().tolist() == [14, 110, 14]
    with pytest.raises(pkg.SourmashError):
        parent.downsample(max_hash=top - 8).norms2()
    # find and compare on the cut never depended on abundances
    assert kept.find(mk(pkg, [20, 31], [1, 1], top - 9), 0.1) == rebuilt(top - 9).find(mk(pkg, [20, 31], [1, 1], top - 9), 0.1)
