"""The pad behind a batch of sequences uploaded from the host.  The sketch kernels load whole 16-byte granules, so they see up
to 15 bytes behind the batch in Engine::seqbuf, a recycled block.  k_protein_fused raises its non-ASCII flag for a byte >= 0x80
there and the host then runs the two-pass path: the same sketch by another route.  The uploads zero the pad, so the route
does not depend on what the block held before.  Here the block holds 0xFF throughout (the pool fill of
tests/test_gpu_pool_fill.py), the batch ends 3 bytes into a granule, and the route assertions of
test_gpu_protein_fused_edges.py::test_runs_of_32 must hold."""
import gc

import pytest

import test_gpu_protein_fused_edges as TP

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ksize", [21, 27])
def test_route_of_a_host_batch_under_a_fill_of_high_bytes(pkg, coracle, ksize):
    L = pkg.lib()
    assert TP.R32_N % 16 != 0                                     # the batch's last granule reaches into the pad
    gc.collect()
    assert L.smh_release_workspace() == 0                         # seqbuf is allocated anew, and filled
    try:
        pkg.matrix.set_pool_fill(0xFF)
        TP.test_runs_of_32(pkg, coracle, ksize)
    finally:
        pkg.matrix.set_pool_fill(-1)
