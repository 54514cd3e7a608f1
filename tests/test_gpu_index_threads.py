"""The index operations from several host threads at once (SURVEY.md "Threading": distinct objects may be used from distinct
threads; test_gpu_sketch.py::test_concurrent_callers pins that for sketching only).  Four threads, each with a resident index
it built itself and a torch stream of its own, run search, nearest, gather, LCA and match on that stream with inputs that are
still being produced when the call is made (tests/stream_order.py); a fifth sketches on a stream of its own.  They share
Device::scratch, the Engine's staging buffers, the block pool and the registry.  Every result equals the restatement's, computed
on one thread beforehand; a refusal on one thread shows in that thread's error slot only; no call takes the device-wide wait
(pool_free_waited).  Once with the pool's test byte (smh_set_pool_fill) and once without.

With the test byte every block the pool hands out is filled and the DEVICE is waited for (device.cpp, pool_fill).  While one
thread sits in that wait the launches of the others are held up, the copy behind a delay they have just queued among them, so a
producer may be over before its thread gets to the call: that run keeps the late inputs but cannot insist that they are still
pending -- its subject is the pattern and the threads, and the wait it adds would hide a wrong stream anyway.  The plain run
insists (stream_order.pending)."""
import ctypes as C
import threading

import numpy as np
import pytest

import search_many_restatement as SR
import stream_order as SO
import test_gpu_stream_order as T

pytestmark = pytest.mark.gpu

THREADS, ROUNDS = 4, 3


@pytest.fixture(scope="module")
def world(pkg, coracle):
    return T.World(pkg, coracle)


@pytest.mark.parametrize("fill", [0x5A, -1], ids=["pool_fill", "plain"])
def test_index_operations_from_four_threads_and_a_sketching_one(pkg, coracle, world, fill):
    import torch
    L = pkg.lib()
    exp = dict(search=world.search(SR.JACCARD, 0.02, 0), nearest=world.nearest(3, SR.MAX_CONTAINMENT, 0.0, 0), gather=world.gather(2, 6),
               lca=[(list(p), per) for p, per in world.lca()], match=world.match(),
               sketch=world.both("sketch", lambda w: T.oracle_state(coracle, world.records[w])))
    total = int(world.rec_off[-1])
    errs, slots = [], [None] * THREADS
    keep = []                                            # indexes and sketches die behind the device-wide wait, by design: not in here
    barrier = threading.Barrier(THREADS + 1)
    old_fill = pkg.matrix.pool_fill()
    waited = {}

    def phase(name):
        """everybody is here; one thread reads the counter.  The rounds lie between "built" and "done": building an index
        and reading a sketch back (its state leaves HBM) free blocks behind the device-wide wait by design, the rounds must not."""
        if barrier.wait(60) == 0:
            waited[name] = T.count(pkg, "pool_free_waited")
        barrier.wait(60)
    insist = SO.pending if fill < 0 else (lambda ev: None)

    def index_thread(i):
        stream = torch.cuda.Stream()
        handle = stream.cuda_stream
        idx = world.index()
        keep.append(idx)
        for k in range(ROUNDS + 1):
            # round 0 is a warm-up in front of the count: the grow-only staging buffers the threads share reach their size,
            # and a regrowth frees the old block behind the device-wide wait (which also holds up the other threads' launches)
            if k == 1:
                phase("built")
            pending = insist if k else (lambda ev: None)
            q = world.late_queries(stream)
            pending(q.ev)
            assert T.search_rows(idx.search_block_dev(q.ptr, world.q_off, 0.02, "jaccard", stream=handle)) == exp["search"]
            q.again()
            pending(q.ev)
            assert T.search_rows(idx.nearest_block_dev(q.ptr, world.q_off, 3, "max_containment", 0.0, stream=handle)) == exp["nearest"]
            a = T.Late(stream, world.q_abunds[0], world.q_abunds[1], armed=False)
            T.arm(q, a)
            pending(q.ev)
            assert T.gather_call(pkg, idx, q.ptr, a.ptr, world.q_off, 2, 6, handle) == exp["gather"]
            q.again()
            pending(q.ev)
            got = idx.lca_counts_block_dev(q.ptr, world.q_off, hash_taxon=True, stream=handle)
            assert [(list(zip(t.tolist(), c.tolist())), per.tolist()) for t, c, per in got] == exp["lca"]
            r = world.late_records(stream)
            pending(r.ev)
            got = idx.match((r.ptr, total, world.rec_off), hits=True, stream=handle)
            rows, offsets, flat = exp["match"]
            assert [tuple(int(col[k]) for col in got[:6]) for k in range(16)] == rows
            assert got.hit_offsets.tolist() == offsets and got.hit_hashes.tolist() == flat
        phase("done")
        # a refusal on thread 0 -- a NaN threshold, decided before the device is touched -- and everybody's error slot
        L.sourmash_err_clear()
        if i == 0:
            q = T.dev(world.q_flat[0])
            row_off = np.zeros(9, dtype=np.uint64)
            rows_p = C.POINTER(pkg._lib.SmhSearchRow)()
            rc = L.smh_index_search_block_dev(idx._h, C.c_void_p(q.data_ptr()), world.q_off.ctypes.data_as(T.u64p), 8, 0, float("nan"), 0,
                                              row_off.ctypes.data_as(T.u64p), C.byref(rows_p), C.c_void_p(handle))
            assert rc == 3
        barrier.wait(60)
        slots[i] = L.sourmash_err_get_last_code()
        barrier.wait(60)
        L.sourmash_err_clear()

    def sketch_thread():
        stream = torch.cuda.Stream()
        mine = []
        for k in range(ROUNDS + 1):
            if k == 1:
                phase("built")
            r = world.late_records(stream)
            mh = pkg.KmerMinHash(*T.SKETCH)
            mine.append(mh)
            (insist if k else (lambda ev: None))(r.ev)
            mh.add_sequences_dev(r.ptr, total, world.rec_off, True, stream.cuda_stream)
        phase("done")
        barrier.wait(60)
        barrier.wait(60)
        for mh in mine:
            assert T.state(mh) == exp["sketch"]

    def guarded(fn, *args):
        try:
            fn(*args)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
            barrier.abort()

    try:
        pkg.matrix.set_pool_fill(fill)
        th = [threading.Thread(target=guarded, args=(index_thread, i)) for i in range(THREADS)]
        th.append(threading.Thread(target=guarded, args=(sketch_thread,)))
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()
    finally:
        pkg.matrix.set_pool_fill(old_fill)
    assert not errs, errs
    assert slots == [3] + [0] * (THREADS - 1)
    assert waited["done"] == waited["built"]
    del keep


def test_a_match_between_small_sketches_takes_no_device_wide_wait(pkg, coracle, world):
    """What the threads above found, from one thread.  The small fold hands the Engine's run buffers over to the sketch it
    leaves in HBM; a match of a few records then sized them anew for its own few runs, and the next small fold had to grow
    them -- a regrowth gives the old block back behind the device-wide wait: two such waits per alternation.  Every caller
    now sizes them for the small fold at least (Engine::ensure_runs), so the counter stands still."""
    idx = world.index()
    seq = T.dev(world.rec_bytes[0])
    total = int(world.rec_off[-1])
    keep = []

    def sketch():
        mh = pkg.KmerMinHash(*T.SKETCH)
        mh.add_sequences_dev(seq.data_ptr(), total, world.rec_off, True)
        keep.append(mh)

    def match():
        return idx.match((seq.data_ptr(), total, world.rec_off))

    sketch(); match(); sketch()                          # every buffer has reached its size
    waited = T.count(pkg, "pool_free_waited")
    for _ in range(3):
        rows = match()
        sketch()
    assert T.count(pkg, "pool_free_waited") == waited
    assert [tuple(int(col[k]) for col in rows[:6]) for k in range(16)] == world.match()[0]
    assert T.state(keep[-1]) == T.oracle_state(coracle, world.records[0])
