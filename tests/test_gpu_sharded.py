"""GPU parity of the SHARDED all-vs-all matrix (north_star: row blocks across the GPUs of a node): the dictionary
pre-pass split by hash range among `world` owners, pair ownership by the circular-half rule, the exchange of the
mirrored blocks.  The ranks of a job are played one after the other in THIS process on the one GPU of the test box
(distributed.simulate_sharded: the collectives become concatenations; everything else is the code the ranks run);
tests/test_gpu_multirank.py runs real processes over a process group.  Every matrix must equal, bit for bit, the
single-rank matrix and the C oracle (reference src/lib.rs:428-436, 470-508)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL = ("jaccard", "common", "size", "count_common", "containment")


def _collection(kind, n, num):
    from sourmash_rust_amd import synth
    if kind == "one_family":
        return synth.family_signatures(0, n, num=num, n_families=1, pool=2 * num, private=num // 2, seed=17)
    sigs = synth.family_signatures(0, n, num=num, n_families=7, pool=2 * num, private=num // 2, seed=17)
    if kind == "one_component":
        sigs[:, 0] = 1          # a contaminant k-mer held by every signature
    return sigs


def _oracle_rows(coracle, sigs, rows, num):
    cols = [sigs[j] for j in range(sigs.shape[0])]
    common, size, jac = coracle.compare_matrix([sigs[i] for i in rows], cols, num, 31, 0)
    return common, size, jac


@pytest.mark.parametrize("tune", [dict(), dict(route="tiled"), dict(route="components"), dict(route="tiled", split_frequent=False)],
                         ids=["auto", "tiled", "components", "tiled-no-split"])
@pytest.mark.parametrize("kind", ["families", "one_component", "one_family"])
@pytest.mark.parametrize("world,n", [(2, 333), (3, 400), (4, 333), (8, 400), (8, 5)])
def test_sharded_matrix_equals_single_rank_and_oracle(world, n, kind, tune, pkg, coracle):
    import torch
    from sourmash_rust_amd import distributed as D
    num = 300
    sigs = _collection(kind, n, num)
    t = torch.from_numpy(sigs.view(np.int64)).cuda()
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(num)
    single = pkg.matrix.compare_block_dev(t, off, t, off, num, want=ALL)
    with pkg.matrix.tuning(**tune):
        outs = D.simulate_sharded(t, n, num, world, want=ALL)
        outs_ns = D.simulate_sharded(t, n, num, world, want=("jaccard", "containment"), symmetric=False)
    blocks = [D.shard_range(n, world, r)[:2] for r in range(world)]
    for name in ALL:
        got = torch.cat([o[name] for o in outs], dim=0)
        assert got.shape == single[name].shape
        assert bool((got == single[name]).all()), (name, world, kind, tune)
    assert bool((torch.cat([o["jaccard"] for o in outs_ns]) == single["jaccard"]).all())
    assert bool((torch.cat([o["containment"] for o in outs_ns]) == single["containment"]).all())
    assert [tuple(o["jaccard"].shape) for o in outs] == [(hi - lo, n) for lo, hi in blocks]
    rows = sorted(set([0, n // 2, n - 1] + list(range(1, n, max(1, n // 9)))))
    ocommon, osize, ojac = _oracle_rows(coracle, sigs, rows, num)
    idx = torch.tensor(rows, device="cuda")
    assert (single["jaccard"][idx].cpu().numpy() == ojac).all()
    assert (single["common"][idx].cpu().numpy().view(np.uint64) == ocommon).all()
    assert (single["size"][idx].cpu().numpy().view(np.uint64) == osize).all()


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_sharded_dictionary_on_ragged_and_skewed_sketches(world, pkg, coracle):
    """The dictionary slices on what the fixed-width benchmark collection never shows: ragged sketches (0 ... 900
    hashes, some EMPTY), hash values crowded into a corner of hash space (bottom-num sketches of genomes of very
    different sizes), heavy duplication across sketches, one hash held by everybody.  Every simulated rank computes
    its row block with ownership 0 (every pair) and with ownership 2 (owned pairs + own diagonal block + pairs that
    share nothing are final): both against the oracle."""
    import torch
    from sourmash_rust_amd import distributed as D, matrix as MX
    rng = np.random.RandomState(77 + world)
    n = 157
    pools = [np.unique(rng.randint(0, 1 << 62, size=1500, dtype=np.int64).astype(np.uint64) >> np.uint64(rng.choice([0, 8, 20, 33])))
             for _ in range(5)]
    sks = []
    for i in range(n):
        pool = pools[i % 5]
        k = int(rng.choice([0, 1, 17, 300, 900]))
        s = np.sort(rng.choice(pool, min(k, pool.size), replace=False)) if k else np.zeros(0, np.uint64)
        if k and i % 3:
            s = np.unique(np.concatenate([s, np.array([12345], dtype=np.uint64)]))      # a hash most sketches hold
        sks.append(s.astype(np.uint64))
    flat, off = MX.csr_from_sketches(sks)
    t = torch.from_numpy(flat.view(np.int64)).cuda()
    for num in (0, 250):
        common, size, jac = coracle.compare_matrix(sks, sks, num, 31, 0)
        colls = [MX.Collection(t, off, world, r) for r in range(world)]
        gathered = None
        if world > 1:
            gathered = torch.empty(world * colls[0].share_bytes, dtype=torch.uint8, device="cuda")
            for r, c in enumerate(colls):
                assert c.share_bytes == colls[0].share_bytes
                c.share_to(gathered[r * c.share_bytes:(r + 1) * c.share_bytes])
        for c in colls:
            c.finish(gathered)
        for r, c in enumerate(colls):
            lo, hi, _ = D.shard_range(n, world, r)
            full = c.compare(lo, hi, num, want=("jaccard", "common", "size"), ownership=MX.OWN_ALL)
            assert (full["common"].cpu().numpy().view(np.uint64) == common[lo:hi]).all(), (world, r, num)
            assert (full["size"].cpu().numpy().view(np.uint64) == size[lo:hi]).all()
            jg = full["jaccard"].cpu().numpy()
            assert ((jg == jac[lo:hi]) | (np.isnan(jg) & np.isnan(jac[lo:hi]))).all()
            own = c.compare(lo, hi, num, want=("common",), ownership=MX.OWN_CIRCULAR if world > 1 else MX.OWN_TRIANGLE)
            i = np.arange(lo, hi)[:, None]; j = np.arange(n)[None, :]
            final = D.owns(i, j, n) | ((j >= lo) & (j < hi)) if world > 1 else np.ones((hi - lo, n), bool)
            got = own["common"].cpu().numpy().view(np.uint64)
            assert (got[final] == common[lo:hi][final]).all(), (world, r, num)
        for c in colls:
            c.close()


def test_c4_dense_matrix_on_four_simulated_ranks(pkg, coracle):
    """BASELINE configs[3] at full size (10 000 x 10 000, num = 2000) on the collection where EVERY pair has to be
    walked (one family), as four ranks: the row blocks equal the single-rank matrix bit for bit, sampled rows equal the
    oracle, and the four ranks together walk about what one rank walks alone -- symmetry survives the sharding (round 2:
    a rank's row block walked the full square)."""
    import ctypes as C
    import torch
    from sourmash_rust_amd import distributed as D, synth
    n, num, world = 10000, 2000, 4
    sigs = synth.family_signatures(0, n, num=num, n_families=1, seed=3)
    t = torch.from_numpy(sigs.view(np.int64)).cuda()
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(num)
    L = pkg.lib()

    def tiled_ms():
        ms, k = C.c_double(), C.c_uint64()
        L.smh_profile_get(b"compare_tiled", C.byref(ms), C.byref(k))
        return ms.value

    single = pkg.matrix.compare_block_dev(t, off, t, off, num, want=("jaccard",))["jaccard"]      # warm-up + reference
    # (the walked work is compared walk for walk: a single owner's dictionary carries range masks from its build, a sliced
    # one builds them with the first block compare whose plan walks enough pairs -- lazy_go -- so the timing switches them
    # off on both sides; the masked sliced matrices are checked below)
    with pkg.matrix.tuning(range_masks=False):
        L.smh_profile_reset(); L.smh_profile_enable(1)
        nomask = pkg.matrix.compare_block_dev(t, off, t, off, num, want=("jaccard",))["jaccard"]
        one = tiled_ms()
        st1 = pkg.matrix.last_stats()
        L.smh_profile_reset()
        outs = D.simulate_sharded(t, n, num, world, want=("jaccard",))
        four = tiled_ms()
        L.smh_profile_enable(0)
    assert bool((nomask == single).all())
    got = torch.cat([o["jaccard"] for o in outs], dim=0)
    assert bool((got == single).all())
    rows = [0, 1, 2499, 2500, 5000, 7777, 9999]
    _, _, ojac = _oracle_rows(coracle, sigs, rows, num)
    assert (got[torch.tensor(rows, device="cuda")].cpu().numpy() == ojac).all()
    assert st1["route"] == "tiled"
    # the four ranks' tiled kernels together against the one rank's: at most 30 % more (the tiles along the ownership
    # boundary are walked by both sides)
    print("tiled kernel: 1 rank %.2f ms, 4 ranks summed %.2f ms" % (one, four))
    assert four <= 1.3 * one, (one, four)
    # with the masks (default tuning): every rank's slice builds them (k_claim_bits / k_elem_bits / k_mask_max_lazy) and its
    # tiled kernel reads them; the row blocks equal the single-rank matrix
    from sourmash_rust_amd import matrix as MX
    colls = [MX.Collection(t, off, world, r) for r in range(world)]
    gathered = torch.empty(world * colls[0].share_bytes, dtype=torch.uint8, device="cuda")
    for r, c in enumerate(colls):
        c.share_to(gathered[r * c.share_bytes:(r + 1) * c.share_bytes])
    for c in colls:
        c.finish(gathered)
    for r, c in enumerate(colls):
        lo, hi, _ = D.shard_range(n, world, r)
        blk = c.compare(lo, hi, num, want=("jaccard",))["jaccard"]
        st = pkg.matrix.last_stats()
        assert st["route"] == "tiled" and st["range_masks"] == 1, (r, st)
        assert bool((blk == single[lo:hi]).all()), r
        del blk
        c.close()


@pytest.mark.parametrize("world", [1, 3])
def test_collection_degenerate_shapes(world, pkg, coracle):
    """The collection dictionary on the shapes that break assumptions: every sketch EMPTY (no hash at all to slice or sort), one
    sketch, two identical sketches, a single hash shared by all -- through smh_collection_* directly, every owner of the
    (simulated) job, ownership 0 and the job's own mode, against the oracle."""
    import torch
    from sourmash_rust_amd import distributed as D, matrix as MX
    shapes = {
        "all_empty": [np.zeros(0, np.uint64) for _ in range(7)],
        "one_sketch": [np.array([3, 9, 27], dtype=np.uint64)],
        "identical": [np.arange(1, 400, dtype=np.uint64)] * 2,
        "one_shared_hash": [np.array([5], dtype=np.uint64) for _ in range(40)],
        "mostly_empty": [np.zeros(0, np.uint64)] * 5 + [np.array([1, 2, 3], dtype=np.uint64)] + [np.zeros(0, np.uint64)] * 4,
    }
    for name, sks in shapes.items():
        n = len(sks)
        flat, off = MX.csr_from_sketches(sks)
        t = torch.from_numpy(np.concatenate([flat, np.zeros(1, np.uint64)]).view(np.int64)).cuda()    # (never a 0-byte allocation)
        for num in (0, 2):
            common, size, jac = coracle.compare_matrix(sks, sks, num, 31, 0)
            colls = [MX.Collection(t, off, world, r) for r in range(world)]
            gathered = None
            if world > 1:
                gathered = torch.empty(world * colls[0].share_bytes, dtype=torch.uint8, device="cuda")
                for r, c in enumerate(colls):
                    c.share_to(gathered[r * c.share_bytes:(r + 1) * c.share_bytes])
            for r, c in enumerate(colls):
                c.finish(gathered)
                lo, hi, _ = D.shard_range(n, world, r)
                full = c.compare(lo, hi, num, want=("common", "size", "jaccard"), ownership=MX.OWN_ALL)
                assert (full["common"].cpu().numpy().view(np.uint64) == common[lo:hi]).all(), (name, world, r, num)
                assert (full["size"].cpu().numpy().view(np.uint64) == size[lo:hi]).all(), (name, world, r, num)
                assert (full["jaccard"].cpu().numpy() == jac[lo:hi]).all(), (name, world, r, num)
                c.close()
            if world > 1 and n >= 2:
                outs = D.simulate_sharded((t, off), n, num, world, want=("common", "jaccard"))
                got = torch.cat([o["common"] for o in outs]).cpu().numpy().view(np.uint64)
                assert (got == common).all(), (name, world, num)


def test_open_dictionary_work_is_ordered_before_calls_on_other_streams(pkg):
    """smh_collection_begin (world 1) and smh_collection_finish (no gathered buffer) return with their kernels still queued
    on the caller's stream A.  A call that follows on ANOTHER stream B rewrites the library's shared pre-pass scratch; it
    must be ordered behind the open work (Device::leave_open / order_after_open), or the first dictionary is silently
    corrupt.  A large collection on stream A (milliseconds of dictionary work), at once a block compare of a different
    collection on stream B, then the first collection's matrix: equal to the one computed with nothing in between."""
    import torch
    from sourmash_rust_amd import synth
    num, n = 2000, 6000
    sigs = synth.family_signatures(0, n, num=num, seed=41)
    other = synth.family_signatures(0, 900, num=num, n_families=1, seed=43)
    t = torch.from_numpy(sigs.view(np.int64)).cuda()
    to = torch.from_numpy(other.view(np.int64)).cuda()
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(num)
    offo = np.arange(901, dtype=np.uint64) * np.uint64(num)
    rows = (2950, 3050)
    quiet = pkg.matrix.Collection(t, off)
    quiet.finish(None)
    want = quiet.compare(rows[0], rows[1], num, want=("jaccard", "common"))
    ref_other = pkg.matrix.compare_block_dev(to, offo, to, offo, num, want=("jaccard",))["jaccard"].clone()
    quiet.close()
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        coll = pkg.matrix.Collection(t, off, stream=sa.cuda_stream)       # returns at once: work open on stream A
        coll.finish(None)
        got_other = pkg.matrix.compare_block_dev(to, offo, to, offo, num, want=("jaccard",), stream=sb.cuda_stream)["jaccard"]
        got = coll.compare(rows[0], rows[1], num, want=("jaccard", "common"))
        assert bool((got["jaccard"] == want["jaccard"]).all()) and bool((got["common"] == want["common"]).all())
        assert bool((got_other == ref_other).all())
        coll.close()


def test_export_dev_says_so_when_the_buffer_is_too_small(pkg):
    import torch
    from sourmash_rust_amd.errors import SourmashError
    mh = pkg.KmerMinHash(0, 21, False, 42, (1 << 64) // 20, True)
    mh.add_many(np.arange(1, 5000, dtype=np.uint64) * np.uint64(1 << 40))
    n = mh.export_dev()
    assert n == len(mh) > 100
    small = torch.full((n - 1,), -1, dtype=torch.int64, device="cuda")
    with pytest.raises(SourmashError) as e:
        mh.export_dev(small, None)
    assert e.value.code == 2 and "capacity" in e.value.message and bool((small == -1).all())
    m = torch.empty(n, dtype=torch.int64, device="cuda")
    a = torch.empty(n, dtype=torch.int64, device="cuda")
    assert mh.export_dev(m, a) == n and (m.cpu().numpy().view(np.uint64) == mh.mins_np()).all()
    num_sketch = pkg.KmerMinHash(10, 21)
    with pytest.raises(SourmashError):
        num_sketch.export_dev()


def test_resident_index_dictionary_can_be_dropped(pkg, coracle):
    from sourmash_rust_amd import synth
    sigs = synth.family_signatures(0, 200, num=300, n_families=3, pool=600, private=150, seed=3)
    nodes = []
    for i in range(200):
        g = pkg.KmerMinHash(300, 31)
        g.add_many(sigs[i])
        nodes.append(g)
    idx = pkg.index.ResidentIndex(nodes)
    a = idx.compare(idx, want=("jaccard",))["jaccard"].copy()
    idx.drop_dictionary()
    b = idx.compare(idx, want=("jaccard",))["jaccard"].copy()       # rebuilt
    assert pkg.lib().smh_release_workspace() == 0                    # drops it again, with the workspace
    c = idx.compare(idx, want=("jaccard",))["jaccard"]
    assert (a == b).all() and (a == c).all()
    rows = [sigs[i] for i in range(200)]
    _, _, jac = coracle.compare_matrix(rows[:20], rows, 300, 31, 0)
    assert (a[:20] == jac).all()
