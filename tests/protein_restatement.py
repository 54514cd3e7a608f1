"""What the protein sketch tests lean on, restated in plain Python / numpy (DESIGN.md "protein arm"; reference
src/lib.rs:252-305).

No product import (same_state and route_counters are handed the package by the GPU tests).  test_protein_field_rules.py
checks every function here against the C oracle or against the layout rule it restates; tests/test_gpu_protein_fused_edges.py and tests/test_gpu_protein_routes.py build their inputs with it.

Six-frame layout: record r owns segments 6r .. 6r+5 = (frame 0 forward, frame 0 reverse complement, frame 1 forward,
frame 1 rc, frame 2 forward, frame 2 rc); frame f of a record of `n` bases holds (n - f) // 3 residues on each strand; a
record shorter than ksize holds none (src/lib.rs:257)."""
import numpy as np

FILLER = 16                     # bases of a filler record: shorter than every protein ksize under test (21, 27, 30)


def rand_dna(rng, n, lower=0.0):
    s = bytearray(rng.choice(b"ACGT") for _ in range(n))
    for i in range(n):
        if rng.random() < lower:
            s[i] |= 0x20
    return s


def segment_lengths(n, ksize):
    """residues of the six segments of a record of `n` bases"""
    if n < ksize:
        return [0] * 6
    return [(n - f) // 3 if n >= f else 0 for f in (0, 0, 1, 1, 2, 2)]


def segment_table(lens, ksize):
    """start of every segment in the residue space of a batch of records (6 * len(lens) + 1 entries, the last = total)"""
    t = [0]
    for n in lens:
        for s in segment_lengths(n, ksize):
            t.append(t[-1] + s)
    return t


def reclen_with_segment_end(seg, j, ksize, lo, base=0):
    """the first record length >= lo whose segment `seg` (0..5) ends at offset `j` of a run of 8 window starts, the
    record's residues starting at `base` of the residue space; None when no length does.  The GPU sweep does not build its
    inputs with this: it runs 24 consecutive lengths, and this only confirms which offsets those reach.  (A
    reverse-complement segment ends where an even number of segments of pairwise equal length ends: with an even base, at even offsets only.)"""
    for n in range(lo, lo + 24):              # the end of segment 0 moves by one per three bases: 24 lengths reach all
        if (base + sum(segment_lengths(n, ksize)[:seg + 1])) % 8 == j:
            return n
    return None


def window_count(n, ksize):
    """windows of ksize // 3 residues over the six frames of a record of `n` clean bases (both strands)"""
    w = ksize // 3
    if n < ksize:
        return 0
    return sum(2 * max(0, (n - f) // 3 - w + 1) for f in range(3))


def polya_windows_per_strand(n, ksize):
    """poly-A of n bases: every forward window is K * (ksize // 3), every reverse one F * (ksize // 3); how many each"""
    w = ksize // 3
    return sum((n - f) // 3 - w + 1 for f in range(3))


def field_offsets(n, islands):
    """record offsets (uint64, ascending, first 0, last n) of a field of `n` bases: every island (start, end) is one record,
    everything between islands is cut into records of FILLER bases and one shorter one where the gap is no multiple"""
    parts = []
    at = 0
    for s, e in sorted(islands) + [(n, n)]:
        s, e = min(s, n), min(e, n)
        assert s >= at
        if s > at:
            parts.append(np.arange(at, s, FILLER, dtype=np.uint64))
        if e > s:
            parts.append(np.array([s], dtype=np.uint64))
        at = max(at, e)
    parts.append(np.array([n], dtype=np.uint64))
    off = np.concatenate(parts)
    assert (off[1:] > off[:-1]).all()
    return off


def prefix_offsets(off, n):
    """the offsets of the first `n` bases of a field: the record that holds base n - 1 ends at n"""
    assert 0 < n <= int(off[-1])
    return np.append(off[:np.searchsorted(off, np.uint64(n))], np.uint64(n))


def with_cuts(off, cuts):
    """the offsets with more record boundaries put in"""
    cuts = np.asarray(sorted(set(int(c) for c in cuts if 0 < c < int(off[-1]))), dtype=np.uint64)
    if not len(cuts):
        return off
    at = np.searchsorted(off, cuts)
    new = off[at] != cuts                        # (at < len(off): every cut lies below the last offset)
    return np.insert(off, at[new], cuts[new])


def island_records(isl, off_cuts, n):
    """the oracle's input: the records that hold island bases.  `isl` = {start: bytes}; `off_cuts` = boundaries put
    inside islands; the field ends at `n`.  Returned in field order as (start, bytes)."""
    out = []
    for s, d in sorted(isl.items()):
        e = min(s + len(d), n)
        if e <= s:
            continue
        cuts = [s] + sorted(c for c in set(off_cuts) if s < c < e) + [e]
        for a, b in zip(cuts, cuts[1:]):
            out.append((a, bytes(d[a - s:b - s])))
    return out


def same_state(g, o):
    """a library sketch and an oracle sketch hold the same hashes and abundances"""
    for a, b in ((g.mins_np(), o.mins_np()), (g.abunds_np(), o.abunds_np())):
        assert a.shape == b.shape and (a == b).all()


def route_counters(pkg, fn):
    """launches of the three protein routes (protein_fused, translate, hash_windows) and reruns of a chunk (chunk_rerun)
    while `fn` runs"""
    import ctypes as C
    L = pkg.lib()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    try:
        fn()
    finally:
        L.smh_profile_enable(0)
    out = {}
    for name in ("protein_fused", "translate", "hash_windows", "chunk_rerun"):
        ms, n = C.c_double(), C.c_uint64()
        L.smh_profile_get(name.encode(), C.byref(ms), C.byref(n))
        out[name] = n.value
    return out
