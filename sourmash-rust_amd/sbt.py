"""Sequence Bloom Trees (reference src/index/sbt.rs, MHBT = SBT<Node<Nodegraph>, Leaf<Signature>>) and their
Nodegraph nodes (reference src/index/nodegraph.rs), over the additive ABI smh_nodegraph_* / smh_sbt_*.

The tree is resident in HBM: every internal nodegraph and every leaf sketch is uploaded once (load or build), and
find / find_many walk it level by level on the device for a whole batch of queries."""
import ctypes as C

import numpy as np

from ._lib import lib, u64p
from .errors import call, take_str
from .index import search_minhashes, search_minhashes_containment
from .minhash import KmerMinHash


def _u64(values):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.uint64).reshape(-1))
    return a, a.ctypes.data_as(u64p)


class Nodegraph:
    """khmer-style bloom filter: n tables of tablesizes[t] bits, hash h sets bit h % tablesizes[t] of each."""

    def __init__(self, tablesizes, ksize, _ptr=None):
        self._L = lib()
        if _ptr is None:
            a, p = _u64(tablesizes)
            _ptr = call(self._L.smh_nodegraph_new, p, a.size, int(ksize))
        self._p = _ptr

    def __del__(self):
        try:
            self._L.smh_nodegraph_free(self._p)
        except Exception:
            pass

    @classmethod
    def from_buffer(cls, data):
        data = bytes(data)
        return cls(None, None, _ptr=call(lib().smh_nodegraph_load_buffer, data, len(data)))

    @classmethod
    def from_path(cls, path):
        return cls(None, None, _ptr=call(lib().smh_nodegraph_load_path, str(path).encode()))

    def to_bytes(self):
        return take_str(call(self._L.smh_nodegraph_save_buffer, self._p))

    def save(self, path):
        with open(path, "wb") as fh:
            fh.write(self.to_bytes())

    def count(self, h):
        return bool(call(self._L.smh_nodegraph_count, self._p, int(h)))

    def get(self, h):
        return int(call(self._L.smh_nodegraph_get, self._p, int(h)))

    def count_many(self, hashes):
        """count() of every hash in array order, on the device; returns which hashes were new (bool array)"""
        a, p = _u64(hashes)
        out = np.zeros(max(a.size, 1), dtype=np.uint8)
        call(self._L.smh_nodegraph_count_many, self._p, p, a.size, out.ctypes.data_as(C.c_void_p))
        return out[:a.size].astype(bool)

    def get_many(self, hashes):
        a, p = _u64(hashes)
        out = np.zeros(max(a.size, 1), dtype=np.uint8)
        call(self._L.smh_nodegraph_get_many, self._p, p, a.size, out.ctypes.data_as(C.c_void_p))
        return out[:a.size].astype(np.int64)

    def update(self, other):
        call(self._L.smh_nodegraph_update, self._p, other._p)

    def similarity(self, other):
        return call(self._L.smh_nodegraph_similarity, self._p, other._p)

    def containment(self, other):
        return call(self._L.smh_nodegraph_containment, self._p, other._p)

    def tablesizes(self):
        n = self._L.smh_nodegraph_tablesizes(self._p, None)
        out = np.zeros(max(n, 1), dtype=np.uint64)
        self._L.smh_nodegraph_tablesizes(self._p, out.ctypes.data_as(u64p))
        return [int(x) for x in out[:n]]

    def n_occupied_bins(self):
        return int(self._L.smh_nodegraph_n_occupied_bins(self._p))

    def unique_kmers(self):
        return int(self._L.smh_nodegraph_unique_kmers(self._p))


def device_bins(tablesizes, hashes):
    """hashes[i] % tablesizes[t] computed by the device modulo: an (n, n_tables) uint32 array"""
    s, sp = _u64(tablesizes)
    h, hp = _u64(hashes)
    out = np.zeros((max(h.size, 1), max(s.size, 1)), dtype=np.uint32)
    call(lib().smh_nodegraph_bins, sp, s.size, hp, h.size, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out[:h.size, :s.size]


class Leaf:
    """A leaf of the tree: its position and (a copy of) its sketch."""

    def __init__(self, pos, minhash):
        self.pos = pos
        self.minhash = minhash

    def __repr__(self):
        return "Leaf(pos=%d, %d hashes)" % (self.pos, len(self.minhash))


class SBT:
    """A resident SBT: from_path (v5 JSON) or build (leaves at positions of a d-ary tree)."""

    def __init__(self, _ptr):
        self._L = lib()
        self._p = _ptr
        n = self._L.smh_sbt_n_leaves(self._p)
        pos = np.zeros(max(n, 1), dtype=np.uint64)
        call(self._L.smh_sbt_leaf_positions, self._p, pos.ctypes.data_as(u64p))
        self._positions = [int(x) for x in pos[:n]]
        self._leaves = None

    def __del__(self):
        try:
            self._L.smh_sbt_free(self._p)
        except Exception:
            pass

    @classmethod
    def from_path(cls, json_path):
        return cls(call(lib().smh_sbt_load_path, str(json_path).encode()))

    @classmethod
    def build(cls, leaves, tablesizes, ksize=1, d=2, positions=None):
        """leaves: KmerMinHash list; positions default to the last level of the smallest complete d-ary tree that
        holds them, left to right (the leaves' order)."""
        leaves = list(leaves)
        if positions is None:
            positions = default_positions(len(leaves), d)
        pa, pp = _u64(positions)
        sa, sp = _u64(tablesizes)
        arr = (C.c_void_p * max(len(leaves), 1))(*[m._p for m in leaves])
        return cls(call(lib().smh_sbt_build, int(d), pp, arr, len(leaves), sp, sa.size, int(ksize)))

    def save(self, json_path):
        """json_path (NAME.sbt.json) plus the directory .sbt.NAME beside it"""
        call(self._L.smh_sbt_save, self._p, str(json_path).encode())

    def __len__(self):
        return len(self._positions)

    @property
    def n_nodes(self):
        return self._L.smh_sbt_n_nodes(self._p)

    def leaf_positions(self):
        return list(self._positions)

    def leaves(self):
        if self._leaves is None:
            self._leaves = {}
            for i, pos in enumerate(self._positions):
                mh = KmerMinHash(0, 0, _ptr=call(self._L.smh_sbt_leaf_sketch, self._p, i))
                self._leaves[pos] = Leaf(pos, mh)
        return [self._leaves[p] for p in self._positions]

    def find_many(self, queries, threshold, containment=False):
        """For every query, the positions of the leaves SBT::find returns, in its order."""
        queries = list(queries)
        n = len(queries)
        arr = (C.c_void_p * max(n, 1))(*[q._p for q in queries])
        offs = np.zeros(n + 1, dtype=np.uint64)
        pos = u64p()
        call(self._L.smh_sbt_find_many, self._p, arr, n, float(threshold), bool(containment),
             offs.ctypes.data_as(u64p), C.byref(pos))
        total = int(offs[-1])
        flat = np.ctypeslib.as_array(pos, shape=(total,)).copy() if total else np.zeros(0, dtype=np.uint64)
        return [[int(x) for x in flat[offs[i]:offs[i + 1]]] for i in range(n)]

    def find_positions(self, query, threshold, containment=False):
        out = np.zeros(max(len(self._positions), 1), dtype=np.uint64)
        cnt = C.c_uint32()
        call(self._L.smh_sbt_find, self._p, query._p, float(threshold), bool(containment), out.ctypes.data_as(u64p),
             C.byref(cnt))
        return [int(x) for x in out[:cnt.value]]

    def find(self, search_fn, query, threshold):
        """SBT::find (reference src/index/sbt.rs:147-175) with index.search_minhashes or
        index.search_minhashes_containment: the matching leaves in the reference's order."""
        if search_fn is search_minhashes:
            containment = False
        elif search_fn is search_minhashes_containment:
            containment = True
        else:
            raise ValueError("SBT.find takes index.search_minhashes or index.search_minhashes_containment")
        hits = self.find_positions(query, threshold, containment)
        by_pos = {leaf.pos: leaf for leaf in self.leaves()}
        return [by_pos[p] for p in hits]


def default_positions(n, d=2):
    """The last level of the smallest complete d-ary tree with room for n leaves, filled left to right."""
    if n == 0:
        return []
    first, width = 0, 1
    while width < n:
        first = first * d + 1
        width *= d
    return list(range(first, first + n))
