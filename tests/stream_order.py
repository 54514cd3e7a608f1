"""The "late input" harness of tests/test_gpu_stream_order.py and tests/test_gpu_index_threads.py: an input
that is still being produced on a stream when the library is called on that stream.

    late(stream, dst, true_src, decoy_src)    dst holds the decoy now; a bounded delay and then dst.copy_(true_src) are queued
                                              on `stream`; returns the event recorded behind the copy
    late_many(stream, triples)                the same for several buffers of one call, behind one delay
    pending(ev)                               asserts that the producer has NOT finished (called right before the library call)

A library call that reads `dst` without being ordered behind `stream` reads the decoy -- a well-formed input of the same shape,
so the call answers wrongly and never faults.  A plain module, not a conftest: nothing here changes how tests are collected.

The delay is torch.cuda._sleep(cycles), a kernel that spins for a fixed number of device clock ticks and ends: nothing waits
without an end.  cycles_per_ms() measures the tick rate once per process with a pair of events; DELAY_MS is the delay's
length.  gaps holds the host time between queueing each producer and its pending() check, so that a run can report the
longest; the delay must be at least 10 times that (DESIGN.md 3.25 records both, and the test module asserts it)."""
import time

DELAY_MS = 40.0
_state = {"cycles_per_ms": None}
gaps = []          # seconds, one entry per late() ... pending() pair


class LateEvent:
    """the event recorded behind a producer, with the host time at which the producer was queued"""

    def __init__(self, event, queued_at):
        self.event, self.queued_at = event, queued_at

    def query(self):
        return self.event.query()

    def synchronize(self):
        self.event.synchronize()


def cycles_per_ms():
    """device clock ticks of torch.cuda._sleep per millisecond, measured once with events"""
    import torch
    if _state["cycles_per_ms"] is None:
        torch.cuda._sleep(1000)                                   # (warm-up: the first launch loads the kernel)
        torch.cuda.synchronize()
        probe = 1_000_000
        for _ in range(3):                                        # (the tick may be the shader clock or a 100 MHz counter)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(probe)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 2.0:
                break
            probe *= 10
        _state["cycles_per_ms"] = probe / ms
    return _state["cycles_per_ms"]


def delay(stream, ms=None):
    """queues a spin of `ms` milliseconds (DELAY_MS) on `stream`"""
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int((DELAY_MS if ms is None else ms) * cycles_per_ms()))


def late(stream, dst, true_src, decoy_src, ms=None):
    """`dst` gets the decoy at once (waited for); on `stream` a delay and then the true contents are queued.  true_src and
    decoy_src are device tensors of dst's shape that are already complete.  Returns the event behind the producer."""
    return late_many(stream, [(dst, true_src, decoy_src)], ms)


def late_many(stream, triples, ms=None):
    """late() for several buffers of one call -- (dst, true_src, decoy_src) each -- behind ONE delay: every decoy is in place
    and waited for before the producer is queued, and one event stands behind all the copies.  (Two late() calls in a row
    would not do: the second one's wait for its decoy is also a wait for the first one's producer.)"""
    import torch
    cycles_per_ms()                                               # (measured before anything is queued)
    for dst, true_src, decoy_src in triples:
        assert dst.shape == true_src.shape == decoy_src.shape and dst.dtype == true_src.dtype == decoy_src.dtype
        dst.copy_(decoy_src)
    # the decoys were written on the current stream; waiting for that stream alone keeps other host threads out of it (a
    # device-wide wait holds up their launches until it returns, and with them the producers they have just queued)
    torch.cuda.current_stream().synchronize()
    t0 = time.perf_counter()
    delay(stream, ms)
    with torch.cuda.stream(stream):
        for dst, true_src, _ in triples:
            dst.copy_(true_src, non_blocking=True)                # device to device
        ev = torch.cuda.Event()
        ev.record(stream)
    return LateEvent(ev, t0)


def pending(*events):
    """The producers behind `events` are still running: a test whose input had already arrived proves nothing about order,
    so it fails here.  Call it immediately before the library call, with no host wait in between."""
    now = time.perf_counter()
    for ev in events:
        done = ev.query()
        gaps.append(now - ev.queued_at)
        assert not done, "the late input arrived before the library was called: this run shows nothing (host gap %.2f ms of a " \
                         "%.0f ms delay)" % ((now - ev.queued_at) * 1e3, DELAY_MS)


def handle(stream):
    """the `void *stream` argument for a torch stream: None (NULL) for the legacy default stream"""
    return stream.cuda_stream or None
