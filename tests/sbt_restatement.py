"""A plain restatement of the reference's SBT search (src/index/sbt.rs:147-277, src/index/nodegraph.rs, src/index.rs:
131-161, src/index/search.rs) in Python + numpy, for the tests: nodegraph files, bloom filters built from leaves, and
SBT::find's stack walk with search_minhashes / search_minhashes_containment."""
import struct

import numpy as np


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


def bloom(sizes, hashes):
    h = np.asarray(list(hashes), dtype=np.uint64)
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


def find(d, sizes, nodes, leaves, query, threshold, containment):
    """SBT::find.  nodes = {pos: (tables, min_n_below or None)}, leaves = {pos: (mins, num)}, query = mins.
    Returns the matching leaf positions in the reference's order."""
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
            mins, num = leaves[pos]
            if containment:
                value = (len(set(mins) & set(query)) / len(mins)) if mins else float("nan")
            else:
                value = compare(mins, query, num)
            if value > threshold:
                out.append(pos)
    return out
