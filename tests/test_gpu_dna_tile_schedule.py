"""How the rolling DNA kernel's tiles are handed out: a launch has as many workgroups as the chip holds at once, and
when there are more tiles than that the workgroups take their further tiles from a counter word.

Sizes follow from the launcher (launch_dna_hash): below 16 777 216 positions a lane's run is 32 positions and a tile
512 * 32 = 16 384; from 33 554 432 positions on a run is 128 positions and a tile 65 536.  The k <= 32 and k = 51 kernels
keep three 512-lane workgroups per CU resident, 768 on the 256 CUs of an MI355X, so 768 tiles are the last static launch
and 769 the first dynamic one.  Every case asserts through the launch counters dna_tiles_static / dna_tiles_dynamic that
the path it aims at ran, and fails if it did not.

Expected sketches come from the C oracle, computed once per module: the oracle walks the longest input once and its
state is noted where each shorter input ends (a sketch fed a stream piece by piece -- pieces overlapping by k - 1 bases
-- is the sketch of the whole stream)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID = 768                  # resident workgroups of the k = 31 kernel
TILE = 16384                # positions per tile below 16.7 M positions
SIZES = (GRID * TILE - 1, GRID * TILE, GRID * TILE + 1, (GRID + 1) * TILE + 17)
SCALED = (1 << 64) // 1000
SEED_DNA = 5


def _count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


def _paths(pkg):
    return _count(pkg, "dna_tiles_static"), _count(pkg, "dna_tiles_dynamic")


def _same(g, o):
    assert g.mins == o[0]
    assert g.abunds == o[1]


@pytest.fixture(scope="module")
def clean(pkg):
    """the longest case-1 input in HBM and on the host, ACGT only"""
    import torch
    n = SIZES[-1]
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    assert pkg.lib().smh_synth_dna_dev(C.c_void_p(buf.data_ptr()), 0, n, SEED_DNA, 0, None) == 0
    torch.cuda.synchronize()
    return buf, bytes(buf[:n].cpu().numpy())


def _oracle_at(coracle, host, case, sizes):
    """{size: (mins, abunds)} of the prefixes of `host`, one pass of the oracle"""
    k = case[1]
    o, out, done = coracle.MinHash(*case), {}, 0
    for n in sorted(sizes):
        o.add_sequence(host[max(done - (k - 1), 0):n], True)
        done = n
        out[n] = (o.mins, o.abunds)
    return out


@pytest.fixture(scope="module")
def expected(clean, coracle):
    host = clean[1]
    cases = {"scaled31": (0, 31, False, 42, SCALED, True), "num31": (500, 31, False, 42, 0, True)}
    out = {name: _oracle_at(coracle, host, case, SIZES) for name, case in cases.items()}
    for name, case in {"scaled21": (0, 21, False, 42, SCALED, True), "scaled32": (0, 32, False, 42, SCALED, True),
                       "scaled51": (0, 51, False, 42, SCALED, True)}.items():
        out[name] = _oracle_at(coracle, host, case, SIZES[2:3])
    return out


# 1. one tile over the grid
@pytest.mark.parametrize("n", SIZES)
def test_one_tile_over_the_grid(n, clean, expected, pkg):
    buf = clean[0]
    g = pkg.KmerMinHash(0, 31, False, 42, SCALED, True)
    pkg.lib().smh_profile_reset()
    g.add_sequences_dev(buf.data_ptr(), n, [0, n], True)
    static, dynamic = _paths(pkg)
    print("n", n, "static launches", static, "dynamic launches", dynamic)
    if n <= GRID * TILE:
        assert static >= 1 and dynamic == 0
    else:
        assert dynamic >= 1 and static == 0
    _same(g, expected["scaled31"][n])
    g = pkg.KmerMinHash(500, 31, False, 42, 0, True)
    g.add_sequences_dev(buf.data_ptr(), n, [0, n], True)
    _same(g, expected["num31"][n])


# 2. records and dirty bytes across dynamically taken tiles
@pytest.fixture(scope="module")
def records(pkg):
    import torch
    n = 14_000_000
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    assert pkg.lib().smh_synth_dna_dev(C.c_void_p(buf.data_ptr()), 0, n, 9, 100_000, None) == 0   # an N every 10^5 bases
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    cuts = np.sort(rng.choice(np.arange(1, n), size=899, replace=False))    # 900 records of unequal length
    cuts[450] = cuts[449] + 17                                              # ... one of them shorter than k
    off = np.concatenate([[0], np.sort(cuts), [n]]).astype(np.uint64)
    assert len(np.unique(off)) == 901 and np.count_nonzero(off[1:-1] % TILE) > 890
    return buf, bytes(buf[:n].cpu().numpy()), off


@pytest.mark.parametrize("force", [True, False])
def test_records_and_dirty_bytes(force, records, pkg, coracle):
    buf, host, off = records
    case = (0, 31, False, 42, SCALED, True)
    g, o = pkg.KmerMinHash(*case), coracle.MinHash(*case)
    first = None
    for a, b in zip(off[:-1], off[1:]):
        try:
            o.add_sequence(host[int(a):int(b)], force)
        except coracle.OracleError as e:
            first = first or e.message
    pkg.lib().smh_profile_reset()
    if force:
        g.add_sequences_dev(buf.data_ptr(), len(host), off, True)
    else:
        assert first is not None
        with pytest.raises(pkg.SourmashError) as ei:
            g.add_sequences_dev(buf.data_ptr(), len(host), off, False)
        assert ei.value.code == 1101 and ei.value.message.endswith(first)
    static, dynamic = _paths(pkg)
    print("force", force, "static launches", static, "dynamic launches", dynamic)
    assert dynamic >= 1 and static == 0
    _same(g, (o.mins, o.abunds))


# 3. the counter word is reused
def test_counter_reuse(records, pkg):
    buf, host, _ = records
    n = len(host)
    case = (0, 31, False, 42, SCALED, True)
    once, twice, again = pkg.KmerMinHash(*case), pkg.KmerMinHash(*case), pkg.KmerMinHash(*case)
    pkg.lib().smh_profile_reset()
    once.add_sequences_dev(buf.data_ptr(), n, [0, n], True)
    again.add_sequences_dev(buf.data_ptr(), n, [0, n], True)
    for _ in range(2):
        twice.add_sequences_dev(buf.data_ptr(), n, [0, n], True)
    assert _paths(pkg) == (0, 4)
    assert once.mins == again.mins and once.abunds == again.abunds
    assert twice.mins == once.mins and twice.abunds == [2 * a for a in once.abunds]


# 4. many tiles per workgroup, GPU against GPU
def test_many_tiles_per_workgroup(pkg):
    """110 MB: runs of 128, 1 679 tiles for 768 workgroups.  The same bytes added as three pieces of 36.7 MB, which
    still have runs of 128 (more than 33.5 M positions) and at most 768 tiles each: three static launches."""
    import torch
    n, k = 110_000_000, 31
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    assert pkg.lib().smh_synth_dna_dev(C.c_void_p(buf.data_ptr()), 0, n, 21, 0, None) == 0
    torch.cuda.synchronize()
    case = (0, k, False, 42, SCALED, True)
    whole, parts = pkg.KmerMinHash(*case), pkg.KmerMinHash(*case)
    pkg.lib().smh_profile_reset()
    whole.add_sequences_dev(buf.data_ptr(), n, [0, n], True)
    assert _paths(pkg) == (0, 1)
    pkg.lib().smh_profile_reset()
    step = (n + 2) // 3
    for lo in range(0, n, step):
        hi = min(lo + step + k - 1, n)
        parts.add_sequences_dev(buf.data_ptr() + lo, hi - lo, [0, hi - lo], True)
    assert _paths(pkg) == (3, 0)
    assert np.array_equal(whole.mins_np(), parts.mins_np()) and np.array_equal(whole.abunds_np(), parts.abunds_np())
    assert len(whole) > 100_000


# 5. the other instantiations
@pytest.mark.parametrize("k", [21, 32, 51])
def test_other_ksizes(k, clean, expected, pkg):
    buf, n = clean[0], SIZES[2]
    g = pkg.KmerMinHash(0, k, False, 42, SCALED, True)
    pkg.lib().smh_profile_reset()
    g.add_sequences_dev(buf.data_ptr(), n, [0, n], True)
    static, dynamic = _paths(pkg)
    print("k", k, "static launches", static, "dynamic launches", dynamic)
    assert dynamic >= 1 and static == 0
    _same(g, expected["scaled%d" % k][n])
    # one tile fewer: as many tiles as this kernel has resident workgroups too, the static path
    pkg.lib().smh_profile_reset()
    pkg.KmerMinHash(0, k, False, 42, SCALED, True).add_sequences_dev(buf.data_ptr(), SIZES[1], [0, SIZES[1]], True)
    assert _paths(pkg) == (1, 0)


@pytest.mark.parametrize("mode", ["scaled", "num"])
def test_grouped(mode, clean, pkg, coracle):
    """smh_add_sequences_grouped at the case-1 size.  Scaled groups share one launch of the ordinary kernel with
    positions: 769 tiles, dynamic.  Bottom-num groups take the per-record kernel, which has no dynamic path: its 769
    tiles are a static launch."""
    host, n = clean[1], SIZES[2]
    cuts = [0, 3_000_001, 3_000_020, 7_654_321, n]
    recs = [host[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    groups = [0, 1, 1, 0]
    case = (0, 31, False, 42, SCALED, True) if mode == "scaled" else (500, 31, False, 42, 0, False)
    gs, os_ = [pkg.KmerMinHash(*case) for _ in range(2)], [coracle.MinHash(*case) for _ in range(2)]
    pkg.lib().smh_profile_reset()
    pkg.KmerMinHash.add_sequences_grouped(gs, recs, groups, True)
    static, dynamic = _paths(pkg)
    print("grouped", mode, "static launches", static, "dynamic launches", dynamic)
    if mode == "scaled":
        assert dynamic >= 1 and static == 0
    else:
        assert static >= 1 and dynamic == 0
    for r, grp in zip(recs, groups):
        os_[grp].add_sequence(r, True)
    for g, o in zip(gs, os_):
        assert g.mins == o.mins and g.abunds == o.abunds


# 6. the host-input pipeline: 128 MB chunks, ranged launches
def test_host_input_pipeline(pkg):
    import torch
    L = pkg.lib()
    n = 300_000_017
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    assert L.smh_synth_dna_dev(C.c_void_p(buf.data_ptr()), 0, n, 12, 99991, None) == 0
    torch.cuda.synchronize()
    host = buf[:n].cpu().numpy()
    off = np.array([0, n], dtype=np.uint64)
    a, b = pkg.KmerMinHash(0, 31, False, 42, SCALED, True), pkg.KmerMinHash(0, 31, False, 42, SCALED, True)
    L.smh_profile_reset()
    assert L.smh_add_sequences(a._p, host.ctypes.data_as(C.c_char_p), off.ctypes.data_as(C.POINTER(C.c_uint64)), 1, True) == 0
    static, dynamic = _paths(pkg)
    print("host input: static launches", static, "dynamic launches", dynamic)
    assert dynamic >= 3 and static == 0           # the two 128 MB chunks are 2 048 tiles each, the last 31.6 MB 964 tiles of runs of 64
    b.add_sequences_dev(buf.data_ptr(), n, off, True)
    assert np.array_equal(a.mins_np(), b.mins_np()) and np.array_equal(a.abunds_np(), b.abunds_np())
    assert len(a) > 250_000
