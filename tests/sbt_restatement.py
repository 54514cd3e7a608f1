"""A plain restatement of the reference's SBT search (src/index/sbt.rs:147-277, src/index/nodegraph.rs, src/index.rs:
131-161, src/index/search.rs) in Python + numpy, for the tests: nodegraph files, bloom filters built from leaves, and
SBT::find's stack walk with search_minhashes / search_minhashes_containment."""
import struct

import numpy as np


def _u64(hashes):
    if isinstance(hashes, np.ndarray):
        return hashes.astype(np.uint64, copy=False).reshape(-1)
    return np.asarray(list(hashes), dtype=np.uint64)


def load_nodegraph(data):
    """OXLI bytes -> (ksize, n_occupied, sizes, [bool array per table])"""
    assert data[:4] == b"OXLI" and data[4] == 4 and data[5] == 2
    ksize, n_tables, occ = struct.unpack_from("<IBQ", data, 6)
    at = 19
    sizes, tables = [], []
    for _ in range(n_tables):
        (size,) = struct.unpack_from("<Q", data, at)
        at += 8
        nbytes = size // 8 + 1
        bits = np.unpackbits(np.frombuffer(data[at:at + nbytes], dtype=np.uint8), bitorder="little")
        assert not bits[size:].any()
        sizes.append(size)
        tables.append(bits[:size].astype(bool))
        at += nbytes
    return ksize, occ, sizes, tables


def table_bytes(tables):
    """the table payloads as the reader reads them (size // 8 + 1 bytes each), concatenated"""
    out = b""
    for t in tables:
        pad = np.zeros(len(t) // 8 * 8 + 8, dtype=bool)
        pad[:len(t)] = t
        out += np.packbits(pad, bitorder="little").tobytes()
    return out


def nodegraph_bytes(ksize, occupied, sizes, tables):
    """Nodegraph::save (nodegraph.rs:97-129): a table of `size` bits is written as ceil(size / 8) bytes, one byte less
    than load_nodegraph reads when size % 8 == 0"""
    out = b"OXLI" + struct.pack("<BBIBQ", 4, 2, ksize, len(sizes), occupied)
    for s, t in zip(sizes, tables):
        out += struct.pack("<Q", s) + np.packbits(t, bitorder="little").tobytes()
    return out


def count_many(sizes, tables, hashes):
    """Nodegraph::count (nodegraph.rs:34-49) of every hash in array order, per table at once: hash i sets a new bit of
    table t iff that bit was clear before the batch and i is the batch's first hash on it.  Sets the bits in `tables`;
    returns (which hashes were new, newly set bits, new hashes): what count() returns and adds to n_occupied_bins and
    unique_kmers."""
    h = _u64(hashes)
    new = np.zeros(h.size, dtype=bool)
    bits = 0
    for s, t in zip(sizes, tables):
        b = (h % np.uint64(s)).astype(np.int64)
        first = np.unique(b, return_index=True)[1]
        fresh = first[~t[b[first]]]
        new[fresh] = True
        bits += int(fresh.size)
        t[b] = True
    return new, bits, int(new.sum())


def get_many(sizes, tables, hashes):
    """Nodegraph::get of every hash (nodegraph.rs:51-59): its bit is set in every table"""
    h = _u64(hashes)
    ok = np.ones(h.size, dtype=bool)
    for s, t in zip(sizes, tables):
        ok &= t[(h % np.uint64(s)).astype(np.int64)]
    return ok


def bloom(sizes, hashes):
    h = _u64(hashes)
    tables = []
    for s in sizes:
        t = np.zeros(s, dtype=bool)
        if h.size:
            t[(h % np.uint64(s)).astype(np.int64)] = True
        tables.append(t)
    return tables


def matches(sizes, tables, mins):
    """number of query hashes whose bit is set in every table (sum of Nodegraph::get)"""
    h = np.asarray(mins, dtype=np.uint64)
    if h.size == 0:
        return 0
    ok = np.ones(h.size, dtype=bool)
    for s, t in zip(sizes, tables):
        ok &= t[(h % np.uint64(s)).astype(np.int64)]
    return int(ok.sum())


def compare(a, b, num):
    """a.compare(b) (reference src/lib.rs:470-508): a's num truncates the union walk"""
    union = sorted(set(a) | set(b))
    if num:
        union = union[:num]
    sa, sb = set(a), set(b)
    common = sum(1 for x in union if x in sa and x in sb)
    return common / max(1, len(union))


def build_nodes(d, leaves, sizes):
    """{pos: (tables, min_n_below)} for every ancestor of a leaf; leaves = {pos: mins}"""
    below = {}
    for pos, mins in leaves.items():
        p = pos
        while p:
            p = (p - 1) // d
            below.setdefault(p, []).append(pos)
    return {p: (bloom(sizes, [h for lp in lps for h in leaves[lp]]), min(len(leaves[lp]) for lp in lps))
            for p, lps in below.items()}


class LazyNodes:
    """build_nodes' mapping for trees too large to build whole: a node's (tables, min_n_below) is made when a walk
    first asks for it.  Nodes with at least `keep` leaves below (the top of the tree, which every walk crosses) stay
    cached; smaller ones are made again on each visit."""

    def __init__(self, d, leaves, sizes, keep=64):
        self.sizes = list(sizes)
        self.leaves = {p: _u64(m) for p, m in leaves.items()}
        self.below = {}
        for pos in self.leaves:
            p = pos
            while p:
                p = (p - 1) // d
                self.below.setdefault(p, []).append(pos)
        self.keep = keep
        self.cache = {}

    def __contains__(self, pos):
        return pos in self.below

    def __getitem__(self, pos):
        got = self.cache.get(pos)
        if got is None:
            lps = self.below[pos]
            got = (bloom(self.sizes, np.concatenate([self.leaves[p] for p in lps])),
                   min(self.leaves[p].size for p in lps))
            if len(lps) >= self.keep:
                self.cache[pos] = got
        return got


def walk_order(d, positions):
    """The leaves in the order SBT::find meets them when every node passes: the stack pops the last child first, so
    a walk that prunes subtrees meets the leaves it reaches in this relative order."""
    leaves = set(positions)
    nodes = set()
    for pos in positions:
        p = pos
        while p:
            p = (p - 1) // d
            nodes.add(p)
    out = []
    stack = [0]
    while stack:
        pos = stack.pop()
        if pos in nodes:
            stack.extend(d * pos + c + 1 for c in range(d))
        elif pos in leaves:
            out.append(pos)
    return out


def check_code(leaf, query):
    """leaf.check_compatible(query) (src/lib.rs:176-190) on (ksize, is_protein, max_hash, seed) tuples: 0, or the
    error code of the first field that differs (MismatchKSizes 101, MismatchDNAProt 102, MismatchMaxHash 103,
    MismatchSeed 104)"""
    for a, b, code in zip(leaf, query, (101, 102, 103, 104)):
        if a != b:
            return code
    return 0


class Incompatible(Exception):
    """The walk reached a leaf that the query is not compatible with: the leaf's compare / count_common fails its
    check_compatible there and SBT::find stops (src/index.rs:138, 152 unwrap the error)."""

    def __init__(self, pos, code):
        super().__init__("leaf %d: error code %d" % (pos, code))
        self.pos = pos
        self.code = code


def find(d, sizes, nodes, leaves, query, threshold, containment, codes=None):
    """SBT::find.  nodes = {pos: (tables, min_n_below or None)}, leaves = {pos: (mins, num)}, query = mins.
    Returns the matching leaf positions in the reference's order.  codes = {leaf pos: check_code(leaf, query)}, if
    given: the first reached leaf with a nonzero code raises Incompatible."""
    out = []
    visited = set()
    stack = [0]
    nq = len(query)
    while stack:
        pos = stack.pop()
        if pos in visited:
            continue
        visited.add(pos)
        if pos in nodes:
            tables, mnb = nodes[pos]
            if nq == 0:
                value = 0.0
            else:
                m = matches(sizes, tables, query)
                if containment:
                    value = m / nq
                else:
                    if mnb is None:
                        raise KeyError("min_n_below")
                    value = m / mnb if mnb else (float("nan") if m == 0 else float("inf"))
            if value > threshold:
                stack.extend(d * pos + c + 1 for c in range(d))
        elif pos in leaves:
            if codes and codes.get(pos):
                raise Incompatible(pos, codes[pos])
            mins, num = leaves[pos]
            if containment:
                value = (len(set(mins) & set(query)) / len(mins)) if mins else float("nan")
            else:
                value = compare(mins, query, num)
            if value > threshold:
                out.append(pos)
    return out
