"""Every entry point with a `void *stream` argument is ordered on that stream (include/sourmash_amd.h, the opening contract;
DESIGN.md 3.25).  Each call gets an input that is STILL BEING PRODUCED when the call is made (tests/stream_order.py):

  caller   the producer runs on a torch stream A of the caller's (one that does not share the library's hardware queue: the
           `apart` fixture), and A's handle is passed
  null     the producer runs on the legacy default stream (handle 0), and NULL is passed

Until the producer ends the buffer holds a decoy: a well-formed input of the same shape whose answer -- by the same restatement
-- differs from the true one (asserted on the CPU first).  A call that reads too early answers the decoy's question; it never
faults.  Outputs the library leaves in device memory are made late the other way round: the buffer is filled with a sentinel BY
THE PRODUCER, so a call that wrote too early is overwritten; they are read through a clone queued on the same stream.  Every
expected value comes from the restatement the family's own tests use (oracle/, tests/*_restatement.py)."""
import ctypes as C

import numpy as np
import pytest

import amino_restatement as AM
import downsample_restatement as DR
import fastx_restatement as FX
import fold_restatement as FR
import gather_restatement as GR
import index_build_restatement as IB
import lca_restatement as LR
import match_restatement as MR
import nearest_restatement as NR
import search_many_restatement as SR
import stream_order as SO

pytestmark = pytest.mark.gpu

K, MX = 21, (1 << 64) // 10
SHARED = 12345                                   # the hash every node holds
NO = LR.NO_TAXON
PARENT = [0, 0, 0, 1, 1, 2, 3]
SENTINEL = 0x5E5E5E5E5E5E5E5E
u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
REC_LENS = [0, 10, 21, 22, 100, 500, 999, 1000, 1500, 2000, 2500, 3000, 64, 65, 777, 1234]   # one empty, one shorter than K
FIELDS = ("match", "common_remaining", "common_original", "size_match", "abund_sum")
SKETCH = (0, K, False, 42, MX, True)             # the sketches the records are added to


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


def dev(a):
    """a numpy array as a device tensor of its own (64- and 32-bit unsigned go as the signed type torch has)"""
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def both(memo, key, fn):
    """The restatement's answer for the true input (fn(0)), computed once.  The decoy's (fn(1)) must differ: asserted here, on
    the CPU, before anything is asked of the device."""
    if key not in memo:
        memo[key] = (fn(0), fn(1))
    true, decoy = memo[key]
    assert true != decoy, "the decoy of %r asks the same question as the true input" % (key,)
    return true


def arm(*lates):
    """queues the producer of every buffer of ONE call behind one delay (stream_order.late_many); returns the first buffer"""
    ev = SO.late_many(lates[0].stream, [(x.dst, x.true, x.decoy) for x in lates])
    for x in lates:
        x.ev = ev
    return lates[0]


def ordered(pkg, lates, call, read=lambda x: x, frees_behind_the_device=False):
    """call() once with every buffer complete, then with every buffer late; read() of what the late call returned.

    The first call is a warm-up: the library's grow-only buffers (Engine staging, Device::scratch) reach the size this input
    needs, behind the device-wide wait a regrowth takes -- a wait that would cover the producer and hide a wrong stream (under
    the mutant that ignores the caller's stream, the first call of a size survived for exactly that reason).  The late call
    must then take no device-wide wait at all: pool_free_waited stands still across it.  frees_behind_the_device: the two
    calls that give blocks back behind the device-wide wait AFTER their work is complete and waited for -- the parser's
    transient PoolBlocks (records.cpp) and the sketch buffers a union replaces -- are exempt from that count; the mutants
    show that their reads are not covered by it."""
    import torch
    for x in lates:
        x.dst.copy_(x.true)
    torch.cuda.synchronize()
    warm = call()
    arm(*lates)
    waited = count(pkg, "pool_free_waited")
    SO.pending(lates[0].ev)
    got = call()
    assert frees_behind_the_device or count(pkg, "pool_free_waited") == waited, "the call waited for the whole device: its producer was waited for, not ordered"
    out = read(got)
    del warm, got
    return out


class Late:
    """a device buffer whose true contents arrive late on `stream` (stream_order.late); keeps both sources alive"""

    def __init__(self, stream, true_np, decoy_np, armed=True):
        import torch
        self.stream, self.true, self.decoy = stream, dev(true_np), dev(decoy_np)
        self.dst = torch.empty_like(self.true)
        for t in (self.true, self.decoy, self.dst):
            t.record_stream(stream)                      # (torch's allocator: the blocks are in use on `stream` too)
        if armed:
            arm(self)

    def again(self):
        return arm(self)

    @property
    def ptr(self):
        return self.dst.data_ptr()


class LateOut:
    """an output buffer the PRODUCER fills with the sentinel: a call that wrote it too early is overwritten.  read() is a clone
    queued on the same stream, with no host wait in front of it."""

    def __init__(self, stream, shape, dtype, armed=True):
        import torch
        self.stream = stream
        self.dst = torch.zeros(shape, dtype=dtype, device="cuda")
        self.true = torch.full(shape, SENTINEL if dtype == torch.int64 else -7.0 if dtype.is_floating_point else 0x5E, dtype=dtype,
                               device="cuda")
        self.decoy = torch.zeros_like(self.true)
        for t in (self.true, self.decoy, self.dst):
            t.record_stream(stream)
        if armed:
            arm(self)

    @property
    def ptr(self):
        return self.dst.data_ptr()

    def read(self):
        import torch
        with torch.cuda.stream(self.stream):
            got = self.dst.clone()
        return got.cpu().numpy()


def beside(stream, fn, ms=8.0):
    """fn() -- something that queues device work elsewhere and waits for it -- while a short delay is pending on `stream`:
    True when it came back with the delay still running, i.e. its work did not queue up behind `stream`'s"""
    import torch
    torch.cuda.synchronize()
    SO.delay(stream, ms)
    with torch.cuda.stream(stream):
        ev = torch.cuda.Event()
        ev.record(stream)
    fn()
    free = not ev.query()
    torch.cuda.synchronize()
    return free


@pytest.fixture(scope="module")
def apart(pkg):
    """A torch stream whose pending work does not hold up the library's own stream.  HIP maps its streams onto a few hardware
    queues (four by default) and a queue starts its packets in order, so a torch stream that shares the library's queue orders
    the library's work behind its own whatever the library asks for: with such a stream as A a call on the wrong stream is
    physically ordered behind the producer and answers correctly (under the mutant that ignores the caller's stream every
    fourth mode-(a) test survived, in step with torch's round-robin over its stream pool).  The probe: with a short delay
    pending on the candidate, a call on the library's own stream (NULL) that waits for its kernel comes back at once."""
    return aparts(pkg)[0]


_aparts = []


def aparts(pkg):
    """two different streams of that kind (found once per process)"""
    import torch
    if not _aparts:
        buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        held = []                                        # (kept, so that torch's pool moves on to another stream)
        for _ in range(12):
            cand = torch.cuda.Stream()
            held.append(cand)
            if all(cand.cuda_stream != s.cuda_stream for s in _aparts) and \
                    beside(cand, lambda: pkg.errors.call(pkg.lib().smh_synth_dna_dev, C.c_void_p(buf.data_ptr()), 0, 4096, 1, 0, None)):
                _aparts.append(cand)
                if len(_aparts) == 2:
                    break
        if len(_aparts) < 2:
            del _aparts[:]
            pytest.fail("no two torch streams among 12 whose pending work leaves the library's own stream free")
    return _aparts


@pytest.fixture(params=["caller", "null"])
def mode(request, apart):
    """(the stream the late input is produced on, the handle the library is given)"""
    import torch
    stream = apart if request.param == "caller" else torch.cuda.default_stream()
    assert (SO.handle(stream) is None) == (request.param == "null")
    yield stream, SO.handle(stream)
    torch.cuda.synchronize()


class World:
    """40 nodes cut from a 60 000-base genome (230 to 370 hashes each at scaled 10, neighbours overlap, one hash held by all),
    8 queries and 16 records with a decoy each, a taxonomy, and every expected value by the restatements."""

    def __init__(self, pkg, coracle):
        self.pkg = pkg
        self.genome = bytes(coracle.synth_dna(0, 60000, 21))
        self.window = MR.window_hashes(self.genome, K)
        assert len(self.window) == 60000 - K + 1
        self.nodes = [sorted(set(self.seg(i * 1400, i * 1400 + 2300 + (i * 211) % 1400)) | {SHARED}) for i in range(40)]
        assert all(200 <= len(n) <= 400 for n in self.nodes), [len(n) for n in self.nodes]
        self.node_taxon = [(1 + i % 6) if i % 7 else NO for i in range(40)]
        self.owners = MR.owners_of(self.nodes)
        self.like = pkg.KmerMinHash(0, K, False, 42, MX, False)
        # queries: q1 is empty, q3 holds only hashes above max_hash (it hits nothing); the decoys have the same sizes
        miss = sorted(set(h for h in self.window if h > MX))[:150]
        self.queries = [sorted(set(self.seg(0, 5000)) | {SHARED}), [], self.seg(10000, 13000), miss, self.seg(20000, 26000),
                        self.seg(30000, 31000), self.seg(40000, 48000), sorted(set(self.seg(52000, 60000)) | {SHARED})]
        spare = [self.seg(a, a + 14000) for a in (30000, 0, 44000, 3000, 0, 12000, 8000, 20000)]
        rng = np.random.RandomState(11)
        self.decoys = [sorted(s[i] for i in rng.choice(len(s), len(q), replace=False)) for q, s in zip(self.queries, spare)]
        assert [len(d) for d in self.decoys] == [len(q) for q in self.queries] and not self.queries[1]
        self.q_off = np.zeros(9, dtype=np.uint64)
        self.q_off[1:] = np.cumsum([len(q) for q in self.queries])
        self.q_flat = [np.array([h for q in qs for h in q], dtype=np.uint64) for qs in (self.queries, self.decoys)]
        self.q_abunds = [np.array([1 + h % 5 for h in self.q_flat[0]], dtype=np.uint64),
                         np.array([7 + h % 3 for h in self.q_flat[1]], dtype=np.uint64)]
        self.shared = [SR.shared(self.nodes, qs) for qs in (self.queries, self.decoys)]
        assert all(len(self.shared[0][q]) == 40 for q in (0, 7)) and not self.shared[0][1] and not self.shared[0][3]
        # records: true and decoy of the same lengths, from different places of the genome
        self.records = [[self.genome[a + r * 3500:a + r * 3500 + n] for r, n in enumerate(REC_LENS)] for a in (0, 1700)]
        self.rec_off = np.zeros(17, dtype=np.uint64)
        self.rec_off[1:] = np.cumsum(REC_LENS)
        self.rec_bytes = [np.frombuffer(b"".join(rs), dtype=np.uint8).copy() for rs in self.records]
        self.memo = {}

    def seg(self, a, b):
        """the sampled hashes of genome[a:b], ascending and distinct"""
        return sorted(set(h for h in self.window[a:b - K + 1] if h <= MX))

    def index(self):
        """a fresh resident index of the nodes, with the taxonomy"""
        idx = self.pkg.index.ResidentIndex([self.mk(n) for n in self.nodes])
        idx.set_taxonomy(PARENT, self.node_taxon)
        return idx

    def mk(self, hashes):
        mh = self.pkg.KmerMinHash(0, K, False, 42, MX, False)
        if len(hashes):
            mh.add_many(np.array(hashes, dtype=np.uint64))
        return mh

    def both(self, key, fn):
        return both(self.memo, key, fn)

    def late_queries(self, stream, armed=True):
        return Late(stream, self.q_flat[0], self.q_flat[1], armed)

    def late_records(self, stream, armed=True):
        return Late(stream, self.rec_bytes[0], self.rec_bytes[1], armed)

    # ---- what the restatements say
    def search(self, metric, threshold, thc):
        return self.both(("search", metric, threshold, thc), lambda w: SR.select(self.shared[w], metric, threshold, thc))

    def nearest(self, k, metric, threshold, thc):
        return self.both(("nearest", k, metric, threshold, thc), lambda w: NR.select(self.shared[w], k, metric, threshold, thc))

    def gather(self, thr, cap):
        def run(w):
            qs = (self.queries, self.decoys)[w]
            ab = dict(zip(self.q_flat[w].tolist(), self.q_abunds[w].tolist()))
            return [GR.gather(self.nodes, q, ab, thr, cap) for q in qs]
        return self.both(("gather", thr, cap), run)

    def lca(self):
        return self.both("lca", lambda w: [LR.counts(PARENT, self.node_taxon, self.owners, q) for q in (self.queries, self.decoys)[w]])

    def lca_records(self):
        return self.both("lca_records", lambda w: LR.classify_records(PARENT, self.node_taxon, self.owners, self.records[w], K, 42, MX))

    def match(self):
        return self.both("match", lambda w: MR.match(self.records[w], K, 42, MX, self.owners))

    def built(self):
        like = dict(num=0, ksize=K, molecule="DNA", seed=42, max_hash=MX, track=False)
        return self.both("build", lambda w: IB.build(self.records[w], [r % 5 for r in range(16)], 5, like))


@pytest.fixture(scope="module", autouse=True)
def report():
    """when the module is through: the longest host time between queueing a producer and the pending() check in front of the
    library call, printed next to the delay (DESIGN.md 3.25 records both); the delay must be at least ten times the gap"""
    yield
    if SO.gaps:
        assert max(SO.gaps) * 1e3 * 10 <= SO.DELAY_MS, "the delay is less than ten times the longest host gap (%.2f ms)" % (max(SO.gaps) * 1e3)
        print("\nstream_order: longest host gap %.3f ms over %d late inputs; delay %.0f ms; %.0f sleep ticks per ms"
              % (max(SO.gaps) * 1e3, len(SO.gaps), SO.DELAY_MS, SO.cycles_per_ms()))


@pytest.fixture(scope="module")
def world(pkg, coracle):
    return World(pkg, coracle)


@pytest.fixture(scope="module")
def index(world):
    return world.index()


KNOBS = {"defaults": {}, "chunked": dict(search=160, gather=160, lca=700, match=400),
         "chunked_grid3": dict(search=160, gather=160, lca=700, match=400, grid=3)}


@pytest.fixture(params=list(KNOBS))
def knobs(request, pkg):
    """the budgets lowered so that every batched call takes several chunks or folds (8 queries x 40 nodes = 320 counters, 3 237
    query hashes, 17 000 record positions), and the grid cap at 3; restored afterwards"""
    MXm = pkg.matrix
    old = (MXm.search_many_budget(), MXm.gather_many_budget(), MXm.lca_budget(), MXm.match_pair_budget(), MXm.grid_cap())
    k = KNOBS[request.param]
    try:
        if k:
            MXm.set_search_many_budget(k["search"]); MXm.set_gather_many_budget(k["gather"]); MXm.set_lca_budget(k["lca"])
            MXm.set_match_pair_budget(k["match"]); MXm.set_grid_cap(k.get("grid", 0))
        yield request.param
    finally:
        MXm.set_search_many_budget(old[0]); MXm.set_gather_many_budget(old[1]); MXm.set_lca_budget(old[2])
        MXm.set_match_pair_budget(old[3]); MXm.set_grid_cap(old[4])


def search_rows(res):
    return [[(int(res.node[r]), int(res.common[r]), int(res.node_size[r]), int(res.query_size[r]))
             for r in range(int(res.offsets[q]), int(res.offsets[q + 1]))] for q in range(len(res.offsets) - 1)]


# ---------------------------------------------------------------------------------- the harness itself

def test_the_delay_is_real(apart):
    """With the producer pending on stream A, a clone queued on a second stream and waited for reads the decoy: a plain racing
    read of valid memory, which is what a library call on the wrong stream would make.  (The second stream is one that does
    not share A's hardware queue: see `apart`.)"""
    import torch
    a = apart
    late = Late(a, np.arange(4096, dtype=np.uint64), np.arange(4096, dtype=np.uint64) + np.uint64(7), armed=False)

    def racing_read(stream):
        with torch.cuda.stream(stream):
            late.true.clone()                            # (the first clone loads its kernel: not inside the delay)
        stream.synchronize()

    held = [torch.cuda.Stream() for _ in range(8)]
    b = next((c for c in held if c.cuda_stream != a.cuda_stream and beside(a, lambda: racing_read(c))), None)
    assert b is not None, "no second stream runs beside stream A"
    arm(late)
    SO.pending(late.ev)
    with torch.cuda.stream(b):
        seen = late.dst.clone()
    b.synchronize()
    assert not late.ev.query(), "the producer ended while the racing read ran"
    assert bool((seen == late.decoy).all())
    late.ev.synchronize()
    assert bool((late.dst == late.true).all())
    print("stream_order: %.0f sleep ticks per ms, delay %.0f ms" % (SO.cycles_per_ms(), SO.DELAY_MS))


# ---------------------------------------------------------------------------------- the resident index

def test_search_block_dev(pkg, world, index, mode, knobs):
    stream, handle = mode
    for metric, name, threshold, thc in ((SR.JACCARD, "jaccard", 0.02, 0), (SR.CONTAINMENT_QUERY, "containment_query", 0.0, 2)):
        exp = world.search(metric, threshold, thc)
        q = world.late_queries(stream, armed=False)
        got = ordered(pkg, [q], lambda: index.search_block_dev(q.ptr, world.q_off, threshold, name, threshold_common=thc, stream=handle),
                      search_rows)
        assert got == exp


def test_nearest_block_dev(pkg, world, index, mode, knobs):
    stream, handle = mode
    exp = world.nearest(3, SR.MAX_CONTAINMENT, 0.0, 0)
    q = world.late_queries(stream, armed=False)
    assert ordered(pkg, [q], lambda: index.nearest_block_dev(q.ptr, world.q_off, 3, "max_containment", 0.0, stream=handle), search_rows) == exp


def gather_call(pkg, index, hashes, abunds, off, thr, cap, handle):
    L = pkg.lib()
    row_off = np.zeros(len(off), dtype=np.uint64)
    assigned = np.zeros(int(off[-1]), dtype=np.uint32)
    rows_p = C.POINTER(pkg._lib.SmhGatherRow)()
    pkg.errors.call(L.smh_index_gather_block_dev, index._h, C.c_void_p(hashes), C.c_void_p(abunds), off.ctypes.data_as(u64p), len(off) - 1,
                    thr, cap, row_off.ctypes.data_as(u64p), C.byref(rows_p), assigned.ctypes.data_as(u32p), C.c_void_p(handle or 0))
    out = []
    for k in range(len(off) - 1):
        rows = [{f: getattr(rows_p[r], f) for f in FIELDS} for r in range(int(row_off[k]), int(row_off[k + 1]))]
        out.append((rows, assigned[int(off[k]):int(off[k + 1])].tolist()))
    pkg.minhash._free(C.cast(rows_p, C.c_void_p))
    return out


def test_gather_block_dev(pkg, world, index, mode, knobs):
    """hashes and abundances both arrive late"""
    stream, handle = mode
    exp = world.gather(2, 6)
    h = world.late_queries(stream, armed=False)
    a = Late(stream, world.q_abunds[0], world.q_abunds[1], armed=False)
    assert ordered(pkg, [h, a], lambda: gather_call(pkg, index, h.ptr, a.ptr, world.q_off, 2, 6, handle)) == exp


def test_lca_block_dev(pkg, world, index, mode, knobs):
    stream, handle = mode
    exp = world.lca()
    q = world.late_queries(stream, armed=False)
    got = ordered(pkg, [q], lambda: index.lca_counts_block_dev(q.ptr, world.q_off, hash_taxon=True, stream=handle))
    assert [(list(zip(t.tolist(), c.tolist())), per.tolist()) for t, c, per in got] == [(list(p), per) for p, per in exp]


def test_lca_sequences_dev(pkg, world, index, mode, knobs):
    stream, handle = mode
    exp = world.lca_records()
    r = world.late_records(stream, armed=False)
    got = ordered(pkg, [r], lambda: index.lca_classify_records((r.ptr, int(world.rec_off[-1]), world.rec_off), stream=handle))
    assert [tuple(int(col[i]) for col in got) for i in range(16)] == exp


def test_match_sequences_dev_with_hits(pkg, world, index, mode, knobs):
    stream, handle = mode
    rows, offsets, flat = world.match()
    assert sum(1 for row in rows if row[4] != MR.MISS) >= 10
    r = world.late_records(stream, armed=False)
    got = ordered(pkg, [r], lambda: index.match((r.ptr, int(world.rec_off[-1]), world.rec_off), hits=True, stream=handle))
    assert [tuple(int(col[i]) for col in got[:6]) for i in range(16)] == rows
    assert got.hit_offsets.tolist() == offsets and got.hit_hashes.tolist() == flat


def test_index_from_sequences_dev(pkg, world, mode, knobs):
    stream, handle = mode
    offsets, hashes, _ = world.built()
    r = world.late_records(stream, armed=False)
    off, got, _ = ordered(pkg, [r], lambda: pkg.index.ResidentIndex.from_records(
        (r.ptr, int(world.rec_off[-1]), world.rec_off), world.like, groups=[k % 5 for k in range(16)], n_groups=5, stream=handle),
        lambda idx: idx.read())
    assert off.tolist() == offsets and got.tolist() == hashes


# ---------------------------------------------------------------------------------- state built lazily on one stream, used on another

def test_lazy_state_built_on_one_stream_serves_the_others(pkg, world, apart):
    """The hash directory, the LCA table and the self-compare dictionary are built by the first call that needs them, on that
    call's stream, with late input; later calls on a second stream and on NULL find them (no second build, equal rows);
    drop_dictionary / a fresh need rebuilds.  No device-wide wait is taken from the first call on: pool_free_waited stands
    still."""
    import torch
    a, b = aparts(pkg)                                   # (neither shares the library's hardware queue)
    exp_s, exp_l = world.search(SR.JACCARD, 0.02, 0), world.lca()

    def lca_rows(got):
        return [(list(zip(t.tolist(), c.tolist())), per.tolist()) for t, c, per in got]

    # a throwaway index first: the same calls bring the shared grow-only buffers to their size, so that the count below is
    # about this test's index alone, whatever ran before
    spare = world.index()
    qw = dev(world.q_flat[0])
    spare.search_block_dev(qw.data_ptr(), world.q_off, 0.02, "jaccard")
    spare.lca_counts_block_dev(qw.data_ptr(), world.q_off, hash_taxon=True)
    with pkg.matrix.tuning(route="tiled"):
        spare.compare(spare, want=("count_common",))
    idx = world.index()
    waited = count(pkg, "pool_free_waited")

    def calls(stream):
        q = world.late_queries(stream)
        SO.pending(q.ev)
        s = search_rows(idx.search_block_dev(q.ptr, world.q_off, 0.02, "jaccard", stream=SO.handle(stream)))
        q.again()
        SO.pending(q.ev)
        l = lca_rows(idx.lca_counts_block_dev(q.ptr, world.q_off, hash_taxon=True, stream=SO.handle(stream)))
        return s, l

    directory, table = count(pkg, "match_directory_built"), count(pkg, "lca_table_built")
    assert calls(a) == (exp_s, [(list(p), per) for p, per in exp_l])
    assert (count(pkg, "match_directory_built"), count(pkg, "lca_table_built")) == (directory + 1, table + 1)
    for stream in (b, torch.cuda.default_stream()):
        assert calls(stream) == (exp_s, [(list(p), per) for p, per in exp_l])
    assert (count(pkg, "match_directory_built"), count(pkg, "lca_table_built")) == (directory + 1, table + 1)
    # the self-compare dictionary: built by the first all-vs-all of the index with itself, dropped, built again
    built = count(pkg, "index_dictionary_built")
    with pkg.matrix.tuning(route="tiled"):            # (1 600 pairs: the automatic route would not take the dictionary)
        first = idx.compare(idx, want=("count_common",))["count_common"].copy()
        assert count(pkg, "index_dictionary_built") == built + 1
        sets = [set(n) for n in world.nodes]
        assert first.tolist() == [[len(x & y) for y in sets] for x in sets]
        assert (idx.compare(idx, want=("count_common",))["count_common"] == first).all()
        assert count(pkg, "index_dictionary_built") == built + 1
        idx.drop_dictionary()
        assert calls(b) == (exp_s, [(list(p), per) for p, per in exp_l])
        assert (idx.compare(idx, want=("count_common",))["count_common"] == first).all()
        assert count(pkg, "index_dictionary_built") == built + 2
    assert (count(pkg, "match_directory_built"), count(pkg, "lca_table_built")) == (directory + 1, table + 1)
    assert count(pkg, "pool_free_waited") == waited
    del spare


# ---------------------------------------------------------------------------------- sketching

def oracle_state(coracle, records, params=SKETCH):
    o = coracle.MinHash(*params)
    for r in records:
        o.add_sequence(bytes(r), True)
    return o.mins, o.abunds


def state(mh):
    return mh.mins, mh.abunds


def test_add_sequences_dev(pkg, coracle, world, mode):
    stream, handle = mode
    exp = world.both("sketch", lambda w: oracle_state(coracle, world.records[w]))
    r = world.late_records(stream, armed=False)

    def call():
        mh = pkg.KmerMinHash(*SKETCH)
        mh.add_sequences_dev(r.ptr, int(world.rec_off[-1]), world.rec_off, True, handle)
        return mh

    assert ordered(pkg, [r], call, state) == exp


def test_add_sequences_grouped_dev(pkg, coracle, world, mode):
    stream, handle = mode
    groups = [k % 3 for k in range(16)]
    exp = world.both("grouped", lambda w: [oracle_state(coracle, [rec for k, rec in enumerate(world.records[w]) if groups[k] == g])
                                           for g in range(3)])
    r = world.late_records(stream, armed=False)

    def call():
        mhs = [pkg.KmerMinHash(*SKETCH) for _ in range(3)]
        pkg.KmerMinHash.add_sequences_grouped_dev(mhs, r.ptr, int(world.rec_off[-1]), world.rec_off, groups, True, handle)
        return mhs

    assert ordered(pkg, [r], call, lambda mhs: [state(m) for m in mhs]) == exp


def amino_records():
    rng = np.random.RandomState(5)
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    lens = [0, 3, 7, 8, 50, 400, 999, 1500]
    return [[bytes(letters[rng.randint(0, 20, size=n)]) for n in lens] for _ in range(2)], lens


def test_add_proteins_dev(pkg, world, mode):
    stream, handle = mode
    recs, lens = amino_records()
    mx = (1 << 64) // 4

    def restated(w):
        o = AM.amino_sketch(recs[w], "protein", K, 0, mx, True, 42)
        return list(o.mins), list(o.abunds)

    exp = world.both("amino", restated)
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    late = Late(stream, *[np.frombuffer(b"".join(r), dtype=np.uint8).copy() for r in recs], armed=False)

    def call():
        mh = pkg.KmerMinHash(0, K, True, 42, mx, True)
        mh.add_proteins_dev(late.ptr, int(off[-1]), off, handle)
        return mh

    assert ordered(pkg, [late], call, state) == exp


def fastx_text(records, fmt):
    out = []
    for k, rec in enumerate(records):
        if fmt == "fasta":
            out.append(b">r%d\n" % k + b"".join(rec[i:i + 70] + b"\n" for i in range(0, len(rec), 70)))
        else:
            out.append(b"@r%d\n" % k + rec + b"\n+\n" + b"I" * len(rec) + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_records_parse_dev(pkg, coracle, world, mode, fmt):
    """the text arrives late; the decoy is another valid text of the same length"""
    stream, handle = mode
    texts = [fastx_text(world.records[w], fmt) for w in (0, 1)]
    assert len(texts[0]) == len(texts[1])

    def restated(w):
        _, records, spans = FX.parse(texts[w], fmt)
        return [len(r) for r in records], spans, oracle_state(coracle, records)

    lens, spans, exp = world.both(("parse", fmt), restated)
    late = Late(stream, *[np.frombuffer(t, dtype=np.uint8).copy() for t in texts], armed=False)
    recs = ordered(pkg, [late], lambda: pkg.fastx.Records.parse(late.dst, fmt, stream=handle), frees_behind_the_device=True)
    assert np.diff(recs.offsets).tolist() == lens
    start, length = recs.name_spans()
    assert list(zip(start.tolist(), length.tolist())) == spans
    mh = pkg.KmerMinHash(*SKETCH)
    mh.add_records(recs, True)
    assert state(mh) == exp


def test_sketch_absorb_dev(pkg, world, mode):
    """the parts arrive late: two sorted parts in one buffer, with abundances"""
    stream, handle = mode
    base = np.array(world.seg(0, 4000), dtype=np.uint64)
    base_ab = np.array([1 + int(h) % 3 for h in base], dtype=np.uint64)
    parts = [[np.array(world.seg(a, b), dtype=np.uint64) for a, b in ((2000, 6000), (5000, 8000))]]
    parts.append([np.array(world.seg(a, a + 9000)[:len(p)], dtype=np.uint64) for a, p in zip((20000, 1000), parts[0])])
    lens = [len(p) for p in parts[0]]
    assert lens == [len(p) for p in parts[1]]
    abunds = [[np.array([w + 2 + int(h) % 4 for h in p], dtype=np.uint64) for p in ps] for w, ps in enumerate(parts)]

    def restated(w):
        m, a = FR.union_parts(base, base_ab, list(zip(parts[w], abunds[w])))
        return m.tolist(), a.tolist()

    exp = world.both("absorb", restated)
    m = Late(stream, np.concatenate(parts[0]), np.concatenate(parts[1]), armed=False)
    a = Late(stream, np.concatenate(abunds[0]), np.concatenate(abunds[1]), armed=False)
    fresh = []
    for _ in range(2):                                   # (made ahead of the calls: the upload of the base is not their business)
        mh = pkg.KmerMinHash(*SKETCH)
        mh.add_many_with_abund(list(zip(base.tolist(), base_ab.tolist())))
        assert mh.export_dev() == len(base)              # its state lies in HBM now
        fresh.append(mh)

    def call():
        mh = fresh.pop()
        mh.absorb_dev(m.dst, a.dst, [0, lens[0]], lens, handle)
        return mh

    assert ordered(pkg, [m, a], call, state, frees_behind_the_device=True) == exp


def test_sketch_export_dev(pkg, coracle, world, mode):
    """a sketch whose state was left in HBM by add_sequences_dev on ANOTHER stream is exported on this one; the output buffers
    are still being filled with the sentinel when the call is made, and are read by a clone queued behind it"""
    import torch
    stream, handle = mode
    mins, abunds = oracle_state(coracle, world.records[0])
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        seq = dev(world.rec_bytes[0])
    other.synchronize()
    mh = pkg.KmerMinHash(*SKETCH)
    mh.add_sequences_dev(seq.data_ptr(), int(world.rec_off[-1]), world.rec_off, True, other.cuda_stream)
    n = len(mins)
    m, a = LateOut(stream, (n,), torch.int64, armed=False), LateOut(stream, (n,), torch.int64, armed=False)
    assert ordered(pkg, [m, a], lambda: mh.export_dev(m.dst, a.dst, handle)) == n
    assert m.read().view(np.uint64).tolist() == mins and a.read().view(np.uint64).tolist() == abunds


def test_synth_dna_dev_then_add_sequences_dev_on_the_same_stream(pkg, coracle, apart):
    """smh_synth_dna_dev with a caller's stream is the third call that leaves its work queued (include/sourmash_amd.h): an
    add_sequences_dev on the same stream, with no wait in between, sketches the finished bytes -- the benchmark's order.  The
    buffer is still being filled with other valid bases by a producer on that stream when the generator is called: a
    generator that ran anywhere else would be overwritten, so the bytes read back by a clone on the stream pin where it ran."""
    import torch
    n = 300_000
    true = bytes(coracle.synth_dna(0, n, 11, 5000))
    decoy = np.frombuffer(bytes(coracle.synth_dna(0, n, 12, 0)), dtype=np.uint8).copy()
    exp, exp_decoy = oracle_state(coracle, [true]), oracle_state(coracle, [decoy.tobytes()])
    assert exp != exp_decoy
    a = apart
    late = Late(a, decoy, np.full(n, ord("A"), dtype=np.uint8))      # the producer's contents are the decoy's
    SO.pending(late.ev)
    pkg.errors.call(pkg.lib().smh_synth_dna_dev, C.c_void_p(late.ptr), 0, n, 11, 5000, C.c_void_p(a.cuda_stream))
    assert not late.ev.query(), "the generator was waited for"
    mh = pkg.KmerMinHash(*SKETCH)
    mh.add_sequences_dev(late.ptr, n, [0, n], True, a.cuda_stream)
    with torch.cuda.stream(a):
        got = late.dst.clone()
    assert state(mh) == exp
    assert got.cpu().numpy().tobytes() == true
    # NULL: the library's own stream, and the buffer is complete on return
    buf2 = dev(decoy)
    torch.cuda.synchronize()
    pkg.errors.call(pkg.lib().smh_synth_dna_dev, C.c_void_p(buf2.data_ptr()), 0, n, 11, 5000, None)
    with torch.cuda.stream(a):
        got = buf2.clone()
    a.synchronize()
    assert got.cpu().numpy().tobytes() == true


# ---------------------------------------------------------------------------------- matrices

N, WIDTH = 24, 60


class Matrices:
    """24 bottom-60 sketches in 3 families; the decoy is the same collection rotated by one sketch (the same hashes: whatever
    a dictionary is built from, it knows every hash), with abundances for the angular block"""

    def __init__(self, pkg, coracle):
        from sourmash_rust_amd import synth
        sigs = synth.family_signatures(0, N, num=WIDTH, n_families=3, pool=2 * WIDTH, private=WIDTH // 2, seed=23)
        self.sigs = [sigs, np.roll(sigs, 1, axis=0).copy()]
        self.off = np.arange(N + 1, dtype=np.uint64) * np.uint64(WIDTH)
        self.abunds = [(1 + (s % np.uint64(9))).astype(np.uint32) for s in self.sigs]
        self.memo = {}
        self.coracle = coracle

    def both(self, key, fn):
        return both(self.memo, key, fn)

    def compare(self, num):
        def run(w):
            rows = [self.sigs[w][i] for i in range(N)]
            common, size, jac = self.coracle.compare_matrix(rows, rows, num, 31, 0)
            return common.tolist(), size.tolist(), jac.tolist()
        return self.both(("compare", num), run)

    def late(self, stream, armed=True):
        return Late(stream, self.sigs[0].reshape(-1), self.sigs[1].reshape(-1), armed)


@pytest.fixture(scope="module")
def mats(pkg, coracle):
    return Matrices(pkg, coracle)


def test_compare_block_dev(pkg, mats, mode):
    import torch
    stream, handle = mode
    common, size, jac = mats.compare(WIDTH)
    t = mats.late(stream, armed=False)
    outs = [LateOut(stream, (N, N), dt, armed=False) for dt in (torch.float64, torch.int64, torch.int64)]
    ordered(pkg, [t] + outs, lambda: pkg.errors.call(
        pkg.lib().smh_compare_block_dev, C.c_void_p(t.ptr), mats.off.ctypes.data_as(u64p), N, C.c_void_p(t.ptr), mats.off.ctypes.data_as(u64p),
        N, WIDTH, C.c_void_p(outs[0].ptr), C.c_void_p(outs[1].ptr), C.c_void_p(outs[2].ptr), None, None, C.c_void_p(handle or 0)))
    assert outs[0].read().tolist() == jac
    assert outs[1].read().view(np.uint64).tolist() == common and outs[2].read().view(np.uint64).tolist() == size


def test_angular_block_dev(pkg, mats, mode):
    import torch
    import angular_restatement as AR
    import test_gpu_angular as TA
    stream, handle = mode

    def restated(w):
        sk = [dict(zip(mats.sigs[w][i].tolist(), mats.abunds[w][i].tolist())) for i in range(N)]
        return AR.block(sk, sk)

    exp = mats.both("angular", restated)
    h = mats.late(stream, armed=False)
    a = Late(stream, mats.abunds[0].reshape(-1), mats.abunds[1].reshape(-1), armed=False)
    outs = [LateOut(stream, (N, N), dt, armed=False) for dt in (torch.int64, torch.float64, torch.float64)]
    ordered(pkg, [h, a] + outs, lambda: pkg.errors.call(
        pkg.lib().smh_angular_block_dev, C.c_void_p(h.ptr), C.c_void_p(a.ptr), mats.off.ctypes.data_as(u64p), N, C.c_void_p(h.ptr),
        C.c_void_p(a.ptr), mats.off.ctypes.data_as(u64p), N, None, False, C.c_void_p(outs[0].ptr), None, None, C.c_void_p(outs[1].ptr),
        C.c_void_p(outs[2].ptr), C.c_void_p(handle or 0)))
    TA.same(outs[0].read().view(np.uint64), outs[1].read(), outs[2].read(), exp, "late input")


def test_downsample_block_dev(pkg, mats, mode):
    import torch
    stream, handle = mode
    cut = int(np.sort(mats.sigs[0].reshape(-1))[N * WIDTH // 3])

    def restated(w):
        h, a, off = DR.cut_csr(mats.sigs[w].reshape(-1), mats.abunds[w].reshape(-1), mats.off, cut)
        return h.tolist(), a.tolist(), off.tolist()

    hashes, abunds, offsets = mats.both("downsample", restated)
    h = mats.late(stream, armed=False)
    a = Late(stream, mats.abunds[0].reshape(-1), mats.abunds[1].reshape(-1), armed=False)
    oh, oa = LateOut(stream, (N * WIDTH,), torch.int64, armed=False), LateOut(stream, (N * WIDTH,), torch.int32, armed=False)
    _, _, new_off = ordered(pkg, [h, a, oh, oa], lambda: pkg.matrix.downsample_block_dev(h.dst, mats.off, cut, a.dst, oh.dst, oa.dst,
                                                                                          stream=handle or 0))
    assert new_off.tolist() == offsets
    k = offsets[-1]
    assert oh.read().view(np.uint64)[:k].tolist() == hashes and oa.read().view(np.uint32)[:k].tolist() == abunds


def test_collection_of_a_single_owner(pkg, mats, mode):
    """world 1: begin and finish leave their work open on the stream (the two stated exceptions); the hashes arrive late, the
    output is filled with the sentinel late"""
    import torch
    stream, handle = mode
    common, _, jac = mats.compare(WIDTH)
    t = mats.late(stream)
    SO.pending(t.ev)
    coll = pkg.matrix.Collection(t.dst, mats.off, stream=handle or 0)
    coll.finish(None)
    outs = [LateOut(stream, (N, N), dt, armed=False) for dt in (torch.float64, torch.int64)]
    arm(*outs)
    SO.pending(outs[0].ev)
    pkg.errors.call(pkg.lib().smh_collection_compare, coll._p, 0, N, WIDTH, pkg.matrix.OWN_TRIANGLE, C.c_void_p(outs[0].ptr),
                    C.c_void_p(outs[1].ptr), None, None, None, C.c_void_p(handle or 0))
    assert outs[0].read().tolist() == jac and outs[1].read().view(np.uint64).tolist() == common
    coll.close()


def test_collection_of_two_owners_in_one_process(pkg, mats, mode):
    """world 2, the ranks played one after the other as distributed.simulate_sharded plays them.  Late: the hashes at each
    begin, the slot of the gather buffer at each share_to (sentinel), the gathered shares at each finish (the decoy is the
    gathered shares of the rotated collection), the output at each compare (sentinel)."""
    import torch
    from sourmash_rust_amd import distributed as D
    stream, handle = mode
    common, _, _ = mats.compare(WIDTH)
    L = pkg.lib()

    def shares(t):
        """the two ranks' shares of the collection behind the complete tensor t, gathered (waited for)"""
        colls = [pkg.matrix.Collection(t, mats.off, 2, r) for r in range(2)]
        out = torch.zeros(2 * colls[0].share_bytes, dtype=torch.uint8, device="cuda")
        for r, c in enumerate(colls):
            c.share_to(out[r * c.share_bytes:(r + 1) * c.share_bytes])
        torch.cuda.synchronize()
        for c in colls:
            c.close()
        return out

    true_shares, decoy_shares = shares(dev(mats.sigs[0].reshape(-1))), shares(dev(mats.sigs[1].reshape(-1)))
    assert true_shares.shape == decoy_shares.shape and not bool((true_shares == decoy_shares).all())
    t = mats.late(stream)
    colls = []
    for r in range(2):
        if r:
            t.again()
        SO.pending(t.ev)
        colls.append(pkg.matrix.Collection(t.dst, mats.off, 2, r, stream=handle or 0))
    nb = colls[0].share_bytes
    gathered = torch.zeros(2 * nb, dtype=torch.uint8, device="cuda")
    for r, c in enumerate(colls):
        slot = LateOut(stream, (nb,), torch.uint8)
        SO.pending(slot.ev)
        pkg.errors.call(L.smh_collection_share_to, c._p, C.c_void_p(slot.ptr), C.c_void_p(handle or 0))
        got = slot.read()
        assert got.tobytes() == true_shares[r * nb:(r + 1) * nb].cpu().numpy().tobytes(), "share_to wrote before the buffer was its own"
    late_g = Late(stream, true_shares.cpu().numpy(), decoy_shares.cpu().numpy())
    for r, c in enumerate(colls):
        if r:
            late_g.again()
        SO.pending(late_g.ev)
        c.finish(late_g.dst)
    blocks = [D.shard_range(N, 2, r)[:2] for r in range(2)]
    got = []
    for r, c in enumerate(colls):
        lo, hi = blocks[r]
        out = LateOut(stream, (hi - lo, N), torch.int64)
        SO.pending(out.ev)
        pkg.errors.call(L.smh_collection_compare, c._p, lo, hi, WIDTH, pkg.matrix.OWN_ALL, None, C.c_void_p(out.ptr), None, None, None,
                        C.c_void_p(handle or 0))
        got.append(out.read().view(np.uint64))
    assert np.concatenate(got).tolist() == common
    for c in colls:
        c.close()


def test_mirror_pack_and_apply(pkg, mode):
    """The exchange of the mirrored blocks, rank 0 of two, through the C entry points.  Pack: the matrix arrives late and the
    send buffer is filled with the sentinel late.  Apply: the row block (read and written: the entries the sender's rows do not
    own must keep what the producer put there) and the received blocks both arrive late.  The CPU arm of
    distributed.mirror_send_list / mirror_apply is the restatement."""
    import torch
    from sourmash_rust_amd import distributed as D
    stream, handle = mode
    L = pkg.lib()
    n = 37
    blocks = [D.shard_range(n, 2, r)[:2] for r in range(2)]
    (lo, hi), (plo, phi) = blocks
    rng = np.random.RandomState(3)
    mat = [rng.randint(1, 1 << 40, size=(hi - lo, n)).astype(np.int64) for _ in range(2)]          # rank 0's block, true and decoy
    recv = [rng.randint(1, 1 << 40, size=((hi - lo) * (phi - plo),)).astype(np.int64) for _ in range(2)]

    def packed(w):
        return D.mirror_send_list(torch.from_numpy(mat[w]), blocks, 0, n)[1].tolist()

    def applied(w):
        out = torch.from_numpy(mat[w].copy())
        D.mirror_apply(out, [out.new_empty(0), torch.from_numpy(recv[w])], blocks, 0, n)
        return out.tolist()

    exp_pack, exp_apply = both({}, "pack", packed), both({}, "apply", applied)
    assert len(exp_pack) == (hi - lo) * (phi - plo)
    kept = sum(1 for row_a, row_m in zip(exp_apply, mat[0].tolist()) for x, y in zip(row_a[plo:phi], row_m[plo:phi]) if x == y)
    assert 0 < kept < (hi - lo) * (phi - plo), "the block must hold entries the sender owns and entries it does not"
    peer_lo, peer_hi = (C.c_uint32 * 1)(plo), (C.c_uint32 * 1)(phi)
    m = Late(stream, mat[0], mat[1], armed=False)
    send = LateOut(stream, (len(exp_pack),), torch.int64, armed=False)
    ordered(pkg, [m, send], lambda: pkg.errors.call(L.smh_mirror_pack, C.c_void_p(m.ptr), hi - lo, n, peer_lo, peer_hi, 1,
                                                    C.c_void_p(send.ptr), C.c_void_p(handle or 0)))
    assert send.read().tolist() == exp_pack
    out = Late(stream, mat[0], mat[1], armed=False)
    r = Late(stream, recv[0], recv[1], armed=False)
    ordered(pkg, [out, r], lambda: pkg.errors.call(L.smh_mirror_apply, C.c_void_p(out.ptr), lo, hi - lo, n, peer_lo, peer_hi, 1,
                                                   C.c_void_p(r.ptr), C.c_void_p(handle or 0)))
    with torch.cuda.stream(stream):
        got = out.dst.clone()
    assert got.cpu().tolist() == exp_apply
