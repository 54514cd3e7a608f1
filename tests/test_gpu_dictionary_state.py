"""GPU parity of the compare path on PERSISTENT dictionaries: one collection dictionary (matrix.Collection, a ResidentIndex,
the slices of a sharded job) serves many block compares under changing tunings, so what it has built -- the partition
table, the range masks -- must be tracked per dictionary, not per call ("Range masks").  The tuning never
changes a result: every matrix equals the C oracle and the first matrix of its sequence, bit for bit, and
matrix.last_stats()["range_masks"] says whether the tiled kernel read the masks (so that a masked shape that silently
falls back to the walk is seen).  The rule for that flag: 1 exactly when the tiled route served the block with masks asked
for, the dictionary carries them (decided when it was built: one built under range_masks=False walks for life) and they
fit (k_mask_layout); the shapes below are chosen so that they fit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WANT = ("jaccard", "common", "size")
# every way a dictionary can be visited in turn: masks off first (the partition table is built, the masks are not), then on
SEQUENCE = [dict(route="tiled", range_masks=False), dict(route="tiled"), dict(), dict(route="components"),
            dict(route="tiled"), dict(route="tiled", range_masks=False), dict(route="tiled")]


def _np(x):
    a = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return a.view(np.uint64) if a.dtype == np.int64 else a


def _profile_count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name, C.byref(ms), C.byref(k))
    return k.value


def _oracle_rows(coracle, sks, rows, num):
    """coracle.compare_matrix of the given rows against ALL sketches, spread over host threads by row"""
    from concurrent.futures import ThreadPoolExecutor      # ctypes releases the GIL inside the C call
    with ThreadPoolExecutor(max_workers=min(16, len(rows))) as ex:
        res = list(ex.map(lambda r: coracle.compare_matrix([sks[r]], sks, num, 31, 0), rows))
    return {"common": np.concatenate([r[0] for r in res]), "size": np.concatenate([r[1] for r in res]),
            "jaccard": np.concatenate([r[2] for r in res])}


def _check(out, ref, row_idx, what):
    """out: dict of numpy matrices; ref: oracle rows; row_idx: where those rows sit in out"""
    for k in WANT:
        got = out[k][row_idx]
        ok = (got == ref[k]) | (np.isnan(got) & np.isnan(ref[k])) if k == "jaccard" else got == ref[k]
        assert ok.all(), (k, what)


def _run_sequence(pkg, fn, masks, what, seq=SEQUENCE):
    """fn() -> dict of numpy matrices, called under every tuning of seq.  masks: whether the dictionary carries range masks
    that fit.  Every matrix equals the first; range_masks follows the rule of the module docstring."""
    first = None
    for tune in seq:
        with pkg.matrix.tuning(**tune):
            out = fn()
            st = pkg.matrix.last_stats()
        if "route" in tune:
            assert st["route"] == tune["route"], (tune, st, what)
        expect = 1 if (masks and tune.get("range_masks", True) and st["route"] == "tiled") else 0
        assert st["range_masks"] == expect, (tune, st, what)
        if first is None:
            first = out
        for k in WANT:
            assert np.array_equal(out[k], first[k], equal_nan=True), (k, tune, what)
    return first


def _ragged(num, pool_n=4500):
    """the shapes of test_range_masks_with_many_words_per_range_and_cuts_near_a_sketch_end, with pools small enough for the
    masks to fit (up to five words in a range: the kernel's tail loop)"""
    rng = np.random.RandomState(11 + num)
    pools = [np.unique(rng.randint(0, 1 << 62, size=pool_n + 1000, dtype=np.int64).astype(np.uint64))[:pool_n] for _ in range(2)]
    sk = []
    for i in range(150):
        pool = pools[i % 2]
        if i % 7 == 3:
            ln = int(rng.randint(3, 40))
        elif i % 7 == 5:
            ln = int(rng.randint(num + 1, num + 6)) if num else 17
        else:
            ln = int(rng.randint(300, 420))
        sk.append(np.sort(rng.choice(pool, ln, replace=False)))
    for i in range(10):
        sk.append(np.unique(rng.randint(0, 1 << 62, size=200, dtype=np.int64).astype(np.uint64)))
    order = rng.permutation(len(sk))
    sk = [sk[i] for i in order]
    sk.append(np.sort(rng.choice(pools[0], (num + 2) if num else 9, replace=False)))
    return sk


def _device_csr(pkg, sks):
    import torch
    flat, off = pkg.matrix.csr_from_sketches(sks)
    return torch.from_numpy(np.concatenate([flat, np.zeros(1, np.uint64)]).view(np.int64)).cuda(), off


def _family_case(n, num, n_fam, seed):
    from sourmash_rust_amd import synth
    sigs = synth.family_signatures(0, n, num=num, n_families=n_fam, pool=2 * num, private=num // 2, seed=seed)
    return [sigs[i] for i in range(n)]


# (name, sketches, nums, oracle rows): the 50-family collection at the C3 shape; the ragged corners with the cut near a
# sketch's end; a block large enough (> 4 Mi pairs) that the partition table and the masks are made beside the fill
# (early_tables) instead of behind the plan
def _world1_cases():
    from sourmash_rust_amd import synth
    c3 = synth.family_signatures(0, 1000, num=2000, n_families=50)
    yield "c3-families", [c3[i] for i in range(1000)], (2000,), [0, 1, 49, 50, 517, 999]
    yield "ragged", _ragged(150), (150, 0), None
    yield "early-tables", _family_case(2100, 500, 50, 8), (500,), [0, 1, 1049, 2050, 2099]


@pytest.mark.parametrize("case", ["c3-families", "ragged", "early-tables"])
def test_tuning_sequence_on_one_world1_collection(case, pkg, coracle):
    """One matrix.Collection (world 1, built under the default tuning: it carries range masks) compared under every tuning
    in turn -- masks off first, so that the partition table exists before the masks do.  A tiled compare with masks
    afterwards must build them, not read pool memory nobody wrote."""
    from sourmash_rust_amd import matrix as MX
    name, sks, nums, rows = next(c for c in _world1_cases() if c[0] == case)
    n = len(sks)
    t, off = _device_csr(pkg, sks)
    coll = MX.Collection(t, off)
    coll.finish(None)
    try:
        for num in nums:
            ref = _oracle_rows(coracle, sks, rows if rows else list(range(n)), num)
            for own in (MX.OWN_ALL, MX.OWN_TRIANGLE):
                got = _run_sequence(pkg, lambda: {k: _np(v) for k, v in coll.compare(0, n, num, want=WANT, ownership=own).items()},
                                    True, (case, num, own))
                _check(got, ref, rows if rows else slice(None), (case, num, own))
    finally:
        coll.close()
    # a dictionary built with the masks switched off walks for life, also under the default tuning afterwards
    with pkg.matrix.tuning(range_masks=False):
        coll = MX.Collection(t, off)
        coll.finish(None)
    try:
        num = nums[0]
        ref = _oracle_rows(coracle, sks, rows if rows else list(range(n)), num)
        got = _run_sequence(pkg, lambda: {k: _np(v) for k, v in coll.compare(0, n, num, want=WANT).items()}, False, (case, "built-no-masks"),
                            seq=[dict(route="tiled"), dict(), dict(route="tiled", range_masks=False), dict(route="tiled")])
        _check(got, ref, rows if rows else slice(None), (case, "built-no-masks"))
    finally:
        coll.close()


def test_tuning_sequence_on_a_resident_index(pkg, coracle):
    """The ResidentIndex caches its dictionary after the first matrix-style call: the same sequence on it (built with masks
    by a default call first), again after drop_dictionary() (rebuilt by the sequence's first call, masks off: it walks for
    life), and once more after a drop and a default call."""
    sks = _family_case(600, 500, 20, 5)
    nodes = []
    for s in sks:
        g = pkg.KmerMinHash(500, 31)
        g.add_many(s)
        nodes.append(g)
    idx = pkg.index.ResidentIndex(nodes)
    ref = _oracle_rows(coracle, sks, list(range(600)), 500)

    def own():
        return {k: _np(v) for k, v in idx.compare(idx, want=WANT).items()}

    _check(own(), ref, slice(None), "prime")
    _check(_run_sequence(pkg, own, True, "index"), ref, slice(None), "index")
    idx.drop_dictionary()
    _check(_run_sequence(pkg, own, False, "index-rebuilt-without-masks"), ref, slice(None), "index-rebuilt-without-masks")
    idx.drop_dictionary()
    _check(own(), ref, slice(None), "prime-again")
    _check(_run_sequence(pkg, own, True, "index-rebuilt"), ref, slice(None), "index-rebuilt")


def _sliced(pkg, t, off, world):
    import torch
    from sourmash_rust_amd import matrix as MX
    colls = [MX.Collection(t, off, world, r) for r in range(world)]
    sb = colls[0].share_bytes
    gathered = torch.empty(world * sb, dtype=torch.uint8, device="cuda")
    for r, c in enumerate(colls):
        assert c.share_bytes == sb
        c.share_to(gathered[r * sb:(r + 1) * sb])
    for c in colls:
        c.finish(gathered)
    return colls


@pytest.mark.parametrize("world", [2, 4])
def test_tuning_sequence_on_sliced_dictionaries(world, pkg, coracle):
    """The dictionary of a sharded job, every owner's slice built here (Collection(world, rank), share_to, finish): its
    masks are built lazily, by the first block compare whose plan walks enough sharing pairs (lazy_go).  A masks-off tiled
    compare first must not use up that chance: the masks-on compares after it read masks (four families: every rank's
    block has enough sharing pairs).  Row blocks equal the world-1 matrix and the oracle."""
    from sourmash_rust_amd import distributed as D
    num, n = 500, 1000
    sks = _family_case(n, num, 4, 7)
    t, off = _device_csr(pkg, sks)
    single = {k: _np(v) for k, v in pkg.matrix.compare_block_dev(t, off, t, off, num, want=WANT).items()}
    rows = [0, 1, 249, 250, 499, 500, 501, 750, 999]
    ref = _oracle_rows(coracle, sks, rows, num)
    _check(single, ref, rows, "world 1")
    colls = _sliced(pkg, t, off, world)
    try:
        for r, c in enumerate(colls):
            lo, hi, _ = D.shard_range(n, world, r)
            got = _run_sequence(pkg, lambda: {k: _np(v) for k, v in c.compare(lo, hi, num, want=WANT).items()}, True, (world, r))
            for k in WANT:
                assert np.array_equal(got[k], single[k][lo:hi], equal_nan=True), (k, world, r)
    finally:
        for c in colls:
            c.close()


def _tie_group(pool_size):
    """3 000 sketches that all hold the same four neighbouring hashes (12 000 keys that tie in the 32 sorted bits: too many
    for k_tie_sort's LDS sort, the four-pass dictionary gives up), plus a few pool hashes each"""
    rng = np.random.RandomState(9)
    shared = np.array([1 << 40, (1 << 40) + 1, (1 << 40) + 2, (1 << 40) + 5], dtype=np.uint64)
    pool = np.unique(rng.randint(1, 1 << 62, size=pool_size, dtype=np.int64).astype(np.uint64))
    return [np.unique(np.concatenate([shared, rng.choice(pool, int(rng.randint(5, 60)), replace=False)])) for _ in range(3000)]


@pytest.mark.parametrize("world", [2, 4])
def test_sliced_dictionary_rebuilt_when_the_four_pass_sort_gives_up(world, pkg, coracle):
    """The tie group as the ranks of a sharded job: the owner whose slice holds it -- rank 0, the four hashes are the smallest
    of the collection -- sends no void share: it rebuilds its slice with all eight passes (collection_begin), on record in
    the `dictionary_rebuilt` count.  Every rank's block equals the world-1 result and the oracle rows."""
    import torch
    from sourmash_rust_amd import distributed as D, matrix as MX
    sks = _tie_group(200000)
    n, num = len(sks), 30
    t, off = _device_csr(pkg, sks)
    single = {k: _np(v) for k, v in pkg.matrix.compare_block_dev(t, off, t, off, num, want=WANT).items()}
    rows = [0, 1, 1500, 2999]
    _check(single, _oracle_rows(coracle, sks, rows, num), rows, "world 1")
    rebuilt, colls = [], []
    try:
        for r in range(world):
            before = _profile_count(pkg, b"dictionary_rebuilt")
            colls.append(MX.Collection(t, off, world, r))
            rebuilt.append(_profile_count(pkg, b"dictionary_rebuilt") - before)
        assert rebuilt[0] == 1 and all(x in (0, 1) for x in rebuilt), rebuilt
        sb = colls[0].share_bytes
        gathered = torch.empty(world * sb, dtype=torch.uint8, device="cuda")
        for r, c in enumerate(colls):
            c.share_to(gathered[r * sb:(r + 1) * sb])
        for c in colls:
            c.finish(gathered)
        for r, c in enumerate(colls):
            lo, hi, _ = D.shard_range(n, world, r)
            for tune in (dict(), dict(route="tiled"), dict(route="tiled", range_masks=False)):
                with pkg.matrix.tuning(**tune):
                    got = {k: _np(v) for k, v in c.compare(lo, hi, num, want=WANT).items()}
                for k in WANT:
                    assert np.array_equal(got[k], single[k][lo:hi], equal_nan=True), (k, world, r, tune)
    finally:
        for c in colls:
            c.close()


def test_a_void_dictionary_is_not_walked_with_or_without_masks(pkg, coracle):
    """The world-1 tie group on the tiled route, with a pool large enough that its range masks fit: the four-pass dictionary
    is void (its masks are built beside the fill before anyone knows), the plan skips the tiles, the call rebuilds the
    dictionary with all eight passes and runs again -- one rebuild per call, masks on and off, and the oracle's numbers."""
    sks = _tie_group(2000000)
    n, num = len(sks), 30
    t, off = _device_csr(pkg, sks)
    rows = [0, 1, 1500, 2999]
    ref = _oracle_rows(coracle, sks, rows, num)
    for tune, masks in ((dict(route="tiled"), 1), (dict(route="tiled", range_masks=False), 0), (dict(), None)):
        before = _profile_count(pkg, b"dictionary_rebuilt")
        with pkg.matrix.tuning(**tune):
            out = {k: _np(v) for k, v in pkg.matrix.compare_block_dev(t, off, t, off, num, want=WANT).items()}
            st = pkg.matrix.last_stats()
        assert _profile_count(pkg, b"dictionary_rebuilt") == before + 1, tune
        if masks is not None:
            assert st["route"] == "tiled" and st["range_masks"] == masks, (tune, st)
        _check(out, ref, rows, tune)
