"""All-vs-all comparison (the N x N matrix the north star names): the reference has no matrix
entry point -- it is N^2 independent calls of KmerMinHash::compare (src/lib.rs:501-508), see
SURVEY.md 3.4.  Here: one device launch per block through the additive C ABI."""
import ctypes as C

import numpy as np

import contextlib

from ._lib import SmhCompareStats, SmhCompareTuning, f64p, lib, u64p
from .errors import call

ROUTES = {"auto": 0, "wave": 1, "few": 2, "components": 3, "tiled": 4}
DICTIONARIES = {"auto": 0, "full": 1}


@contextlib.contextmanager
def tuning(route="auto", visit_all_tiles=False, use_symmetry=True, comp_pairs_limit=96 << 10, split_frequent=True, dictionary="auto",
           range_masks=True):
    """Pins which kernel serves the block compares inside the `with` (additive ABI
    smh_compare_set_tuning; results never depend on it), then restores the defaults."""
    t = SmhCompareTuning(ROUTES[route], int(visit_all_tiles), int(use_symmetry), comp_pairs_limit, int(split_frequent),
                         DICTIONARIES[dictionary], 0 if range_masks else 1)
    call(lib().smh_compare_set_tuning, C.byref(t))
    try:
        yield
    finally:
        call(lib().smh_compare_set_tuning, None)


def last_stats():
    st = SmhCompareStats()
    lib().smh_compare_last_stats(C.byref(st))
    names = {v: k for k, v in ROUTES.items()}
    return {"route": names.get(st.route, "none"), "rows_per_tile": st.rows_per_tile, "tiles_visited": st.tiles_visited,
            "tiles_total": st.tiles_total, "pairs_per_tile": st.pairs_per_tile, "lds_overflow_steps": st.lds_overflow_steps,
            "frequent_hashes": st.frequent_hashes, "pipelined": st.pipelined,
            "span_halvings": st.span_halvings, "prefetched_after_halving": st.prefetched_after_halving,
            "range_masks": int(lib().smh_compare_last_range_masks())}


def compare_block(rows, cols, want=("jaccard",)):
    """rows/cols: lists of KmerMinHash.  Returns dict name -> (len(rows), len(cols)) array.
    names: jaccard, common, size, count_common, containment."""
    n, m = len(rows), len(cols)
    out = {}
    bufs = {"jaccard": np.float64, "common": np.uint64, "size": np.uint64, "count_common": np.uint64,
            "containment": np.float64}
    for k in want:
        out[k] = np.zeros((n, m), dtype=bufs[k])

    def ptr(name):
        if name not in out:
            return None
        return out[name].ctypes.data_as(f64p if out[name].dtype == np.float64 else u64p)

    R = (C.c_void_p * max(n, 1))(*[r._p for r in rows])
    Cc = (C.c_void_p * max(m, 1))(*[c._p for c in cols])
    call(lib().smh_compare_block, R, n, Cc, m, ptr("jaccard"), ptr("common"), ptr("size"), ptr("count_common"),
         ptr("containment"))
    return out


def csr_from_sketches(sketches):
    """list of ascending uint64 arrays -> (flat uint64 array, uint64 offsets)."""
    off = np.zeros(len(sketches) + 1, dtype=np.uint64)
    for i, s in enumerate(sketches):
        off[i + 1] = off[i] + len(s)
    flat = np.concatenate([np.asarray(s, dtype=np.uint64) for s in sketches]) if sketches else np.zeros(0, np.uint64)
    return np.ascontiguousarray(flat), off


def compare_block_dev(row_hashes, row_offsets, col_hashes, col_offsets, num, want=("jaccard",), stream=None):
    """Device-resident CSR sketches (torch uint64/int64 CUDA tensors) -> dict of CUDA tensors.
    torch is only the allocator here; the work is the library's HIP kernel."""
    import torch
    n, m = len(row_offsets) - 1, len(col_offsets) - 1
    dev = row_hashes.device
    outs = {}
    for k in want:
        dt = torch.float64 if k in ("jaccard", "containment") else torch.int64
        outs[k] = torch.empty((n, m), dtype=dt, device=dev)

    def p(name):
        return C.c_void_p(outs[name].data_ptr()) if name in outs else C.c_void_p(0)

    ro = np.ascontiguousarray(row_offsets, dtype=np.uint64)
    co = np.ascontiguousarray(col_offsets, dtype=np.uint64)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    call(lib().smh_compare_block_dev, C.c_void_p(row_hashes.data_ptr()), ro.ctypes.data_as(u64p), n,
         C.c_void_p(col_hashes.data_ptr()), co.ctypes.data_as(u64p), m, num,
         p("jaccard"), p("common"), p("size"), p("count_common"), p("containment"), C.c_void_p(stream))
    return outs


def angular_block_dev(row_hashes, row_abunds, row_offsets, col_hashes, col_abunds, col_offsets, count_common=None, symmetric=False,
                      want=("angular",), stream=None):
    """Angular similarity of device-resident CSR sketches (smh_angular_block_dev): hashes are uint64/int64 CUDA tensors,
    abundances uint32/int32 CUDA tensors, offsets host arrays.  count_common (optional CUDA int64/uint64 matrix) prunes the
    pairs whose entry is 0.  Returns a dict of CUDA tensors; names: dot, cosine, angular, row_norm2, col_norm2."""
    import torch
    n, m = len(row_offsets) - 1, len(col_offsets) - 1
    dev = row_hashes.device
    kinds = {"dot": (torch.int64, (n, m)), "cosine": (torch.float64, (n, m)), "angular": (torch.float64, (n, m)),
             "row_norm2": (torch.int64, (n,)), "col_norm2": (torch.int64, (m,))}
    outs = {k: torch.empty(kinds[k][1], dtype=kinds[k][0], device=dev) for k in want}

    def p(name):
        return C.c_void_p(outs[name].data_ptr()) if name in outs else C.c_void_p(0)

    ro = np.ascontiguousarray(row_offsets, dtype=np.uint64)
    co = np.ascontiguousarray(col_offsets, dtype=np.uint64)
    if count_common is not None:
        assert count_common.is_contiguous() and tuple(count_common.shape) == (n, m) and count_common.element_size() == 8
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    call(lib().smh_angular_block_dev, C.c_void_p(row_hashes.data_ptr()), C.c_void_p(row_abunds.data_ptr()), ro.ctypes.data_as(u64p), n,
         C.c_void_p(col_hashes.data_ptr()), C.c_void_p(col_abunds.data_ptr()), co.ctypes.data_as(u64p), m,
         C.c_void_p(count_common.data_ptr() if count_common is not None else 0), bool(symmetric),
         p("dot"), p("row_norm2"), p("col_norm2"), p("cosine"), p("angular"), C.c_void_p(stream))
    return outs


def downsample_block_dev(hashes, offsets, max_hash, abunds=None, out_hashes=None, out_abunds=None, stream=None):
    """The kept prefixes (hashes <= max_hash) of device-resident CSR sketches (smh_downsample_block_dev): hashes uint64/int64,
    abundances uint32/int32 CUDA tensors, offsets a host array.  Output tensors are allocated with the input's size when not
    given (their numel is the capacity).  Returns (out_hashes, out_abunds or None, new offsets as a uint64 numpy array); the
    first new_offsets[-1] elements of the outputs are valid."""
    import torch
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = off.size - 1
    dev = hashes.device
    if out_hashes is None:
        out_hashes = torch.empty(max(int(off[-1] - off[0]), 1), dtype=hashes.dtype, device=dev)
    if abunds is not None and out_abunds is None:
        out_abunds = torch.empty(out_hashes.numel(), dtype=abunds.dtype, device=dev)
    cap = out_hashes.numel() if abunds is None else min(out_hashes.numel(), out_abunds.numel())
    new_off = np.zeros(n + 1, dtype=np.uint64)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    call(lib().smh_downsample_block_dev, C.c_void_p(hashes.data_ptr()), C.c_void_p(abunds.data_ptr() if abunds is not None else 0),
         off.ctypes.data_as(u64p), n, int(max_hash), C.c_void_p(out_hashes.data_ptr()),
         C.c_void_p(out_abunds.data_ptr() if abunds is not None else 0), cap, new_off.ctypes.data_as(u64p), C.c_void_p(stream))
    return out_hashes, (out_abunds if abunds is not None else None), new_off


def downsample_geometry():
    """(output elements per workgroup of the copy kernel, its threads)"""
    t, th = C.c_uint32(), C.c_uint32()
    lib().smh_downsample_geometry(C.byref(t), C.byref(th))
    return t.value, th.value


def match_geometry():
    """(owner pairs of a record the tally counts in LDS, threads it gives a record, directory hashes the probe samples into LDS)"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().smh_match_geometry(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def match_pair_budget():
    return int(lib().smh_match_pair_budget())


def set_match_pair_budget(pairs):
    """bounds the work space of ResidentIndex.match (smh_match_set_pair_budget); 0 restores the default"""
    lib().smh_match_set_pair_budget(int(pairs))


def lca_geometry():
    """(owners of a hash one lane folds, distinct sampled hashes of a record one lane folds, threads a longer one gets)"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().smh_lca_geometry(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def lca_budget():
    return int(lib().smh_lca_budget())


def set_lca_budget(keys):
    """the query hashes one chunk of ResidentIndex.lca_counts may hold (smh_lca_set_budget); 0 restores the default"""
    lib().smh_lca_set_budget(int(keys))


def grid_cap():
    return int(lib().smh_grid_cap())


def set_grid_cap(workgroups):
    """at most this many workgroups for the resident-index kernels that loop by the grid (smh_set_grid_cap): a test knob that
    brings the loops' later trips to small shapes -- no result depends on it; 0 restores the default (no cap)"""
    lib().smh_set_grid_cap(int(workgroups))


def pool_fill():
    return int(lib().smh_pool_fill())


def set_pool_fill(byte):
    """fill every device block the library's pool hands out or parks with this byte, 0 .. 255 (smh_set_pool_fill): a test
    knob that puts a known pattern where work space would read zeros or the last call's values -- no result depends on it;
    -1 restores the default (off)"""
    lib().smh_set_pool_fill(int(byte))


def gather_many_budget():
    return int(lib().smh_gather_many_budget())


def set_gather_many_budget(pairs):
    """the (query, node) counters one chunk of ResidentIndex.gather_many may hold (smh_gather_many_set_budget); 0 restores
    the default"""
    lib().smh_gather_many_set_budget(int(pairs))


def search_geometry():
    """(owners of a hash the lane holding a query position walks itself, nodes of one workgroup of the select and emit
    kernels, most queries of a chunk) of ResidentIndex.search_many"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().smh_search_geometry(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def nearest_geometry():
    """(largest k, nodes of one workgroup of the tile kernel, keys the merge sorts at once) of ResidentIndex.nearest / knn
    (smh_nearest_geometry): a query with more than merge_slots - k kept candidates takes more than one merge step"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().smh_nearest_geometry(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def search_many_budget():
    return int(lib().smh_search_many_budget())


def set_search_many_budget(pairs):
    """the (query, node) counters one chunk of ResidentIndex.search_many / pairwise may hold (smh_search_many_set_budget);
    0 restores the default"""
    lib().smh_search_many_set_budget(int(pairs))


def cluster_geometry():
    """(adjacency-list length up to which one lane walks a node's list in a greedy round, nodes of one workgroup of the linking
    pass) of ResidentIndex.cluster"""
    a, b = C.c_uint32(), C.c_uint32()
    lib().smh_cluster_geometry(C.byref(a), C.byref(b))
    return a.value, b.value


def collapse_geometry():
    """(owner-list length up to which one lane folds a hash's owners, up to which one wave does, groups one round of LDS
    counters covers for a longer list) of ResidentIndex.collapse"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().smh_collapse_geometry(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def filter_geometry():
    """(resident hashes one workgroup trip of the flag and emit passes takes, sampled top of the operand the search keeps in
    LDS, threads of the workgroup) of ResidentIndex.filter"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().smh_filter_geometry(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def cluster_pair_budget():
    return int(lib().smh_cluster_pair_budget())


def set_cluster_pair_budget(entries):
    """the directed adjacency entries the greedy linkage of ResidentIndex.cluster may hold (smh_cluster_set_pair_budget);
    0 restores the default"""
    lib().smh_cluster_set_pair_budget(int(entries))


def cluster_rounds():
    return int(lib().smh_cluster_rounds())


def set_cluster_rounds(rounds):
    """the greedy rounds ResidentIndex.cluster queues between two read-backs (smh_cluster_set_rounds); 0 restores the default"""
    lib().smh_cluster_set_rounds(int(rounds))


def angular_last_stats():
    """(pairs walked, pairs given zeros without a walk) of the last angular call"""
    a, b = C.c_uint64(), C.c_uint64()
    lib().smh_angular_last_stats(C.byref(a), C.byref(b))
    return a.value, b.value


OWN_ALL, OWN_TRIANGLE, OWN_CIRCULAR = 0, 1, 2


class Collection:
    """The dictionary of one collection of sketches resident in HBM (additive ABI smh_collection_*): dense ranks of
    all hashes, components, frequent hashes -- built once, by this process alone (world=1) or together with the other
    ranks of a job (each sorts one slice of hash space; ONE all-gather of the shares in between), then any number of
    block compares.  hashes: CUDA int64/uint64 tensor (kept alive by this object); offsets: host uint64 array, n+1."""

    def __init__(self, hashes, offsets, world=1, rank=0, stream=None):
        import torch
        self._hashes = hashes
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.n = len(self.offsets) - 1
        self.world, self.rank = world, rank
        self._stream = stream if stream is not None else torch.cuda.current_stream(hashes.device).cuda_stream
        L = lib()
        self._p = None
        self._p = call(L.smh_collection_begin, C.c_void_p(hashes.data_ptr()), self.offsets.ctypes.data_as(u64p), self.n, world, rank,
                       C.c_void_p(self._stream))
        self.share_bytes = int(L.smh_collection_share_bytes(self._p))

    def share_to(self, dst):
        """copies this rank's share into `dst` (a CUDA uint8 tensor of share_bytes bytes, e.g. its slot of the gather buffer)"""
        assert dst.numel() * dst.element_size() == self.share_bytes and dst.is_contiguous()
        call(lib().smh_collection_share_to, self._p, C.c_void_p(dst.data_ptr()), C.c_void_p(self._stream))

    def finish(self, gathered=None):
        """gathered: CUDA uint8 tensor, world x share_bytes, rank-major (None when world == 1)"""
        if gathered is not None:
            assert gathered.is_contiguous() and gathered.numel() * gathered.element_size() == self.world * self.share_bytes
        self._gathered = gathered
        call(lib().smh_collection_finish, self._p, C.c_void_p(gathered.data_ptr() if gathered is not None else 0),
             C.c_void_p(self._stream))
        self._gathered = None

    def compare(self, row_lo, row_hi, num, want=("jaccard",), ownership=OWN_ALL):
        """rows [row_lo, row_hi) x all columns -> dict name -> CUDA tensor (row_hi - row_lo, n)"""
        import torch
        dev = self._hashes.device
        outs = {}
        for k in want:
            dt = torch.float64 if k in ("jaccard", "containment") else torch.int64
            outs[k] = torch.empty((row_hi - row_lo, self.n), dtype=dt, device=dev)

        def p(name):
            return C.c_void_p(outs[name].data_ptr()) if name in outs and outs[name].numel() else C.c_void_p(0)

        if row_hi > row_lo:
            call(lib().smh_collection_compare, self._p, row_lo, row_hi, num, ownership, p("jaccard"), p("common"), p("size"),
                 p("count_common"), p("containment"), C.c_void_p(self._stream))
        return outs

    def close(self):
        if self._p:
            lib().smh_collection_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
