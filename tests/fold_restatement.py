"""The fold restated in plain numpy (DESIGN.md "fold"; reference src/lib.rs:192-245 for a stream of hashes).

No product import: this is what sort.hip and its host drivers in minhash.cpp are compared against, value for value.  A
sketch's state is (mins, abunds): ascending distinct uint64 hashes and, for a tracked sketch, their uint64 abundances
(None when the sketch does not track them).  test_fold_rules.py checks every function here against the C oracle.

Tracked bottom-num sketches are order-dependent (quirk Q3): they have no model here, the C oracle is their reference."""
import numpy as np

U64 = np.uint64


def _u64(a):
    return np.ascontiguousarray(a, dtype=U64).reshape(-1)


def union_parts(mins, abunds, parts):
    """Set union of the state with `parts` = [(mins_i, abunds_i or None), ...], abundances summed (in uint64): what add_hash,
    hash by hash and abundance times each, gives for a scaled sketch.  abunds None = untracked: returns (mins, None)."""
    track = abunds is not None
    hs = [_u64(mins)] + [_u64(p[0]) for p in parts]
    allh = np.concatenate(hs)
    if not track:
        return np.unique(allh), None
    cs = [_u64(abunds)] + [_u64(p[1]) for p in parts]
    assert all(h.size == c.size for h, c in zip(hs, cs)), "every part of a tracked union carries one abundance per hash"
    uniq, inv = np.unique(allh, return_inverse=True)
    out = np.zeros(uniq.size, dtype=U64)
    np.add.at(out, inv.reshape(-1), np.concatenate(cs))
    return uniq, out


def scaled_add(mins, abunds, hashes, max_hash, track):
    """add_many(hashes) into a scaled sketch: the hashes <= max_hash, distinct, with their number of occurrences, united
    with the state."""
    h = _u64(hashes)
    h = h[h <= U64(max_hash)]
    uniq, cnt = np.unique(h, return_counts=True)
    if not track:
        return union_parts(mins, None, [(uniq, None)])
    return union_parts(mins, _u64(abunds if abunds is not None else []), [(uniq, cnt.astype(U64))])


def num_add_untracked(mins, hashes, num):
    """add_many(hashes) into an untracked bottom-num sketch: the `num` smallest of the union"""
    return np.unique(np.concatenate([_u64(mins), _u64(hashes)]))[:num]


def check_sorted_with_payload(keys_in, keys_out, payload_out):
    """O(n) verdict on a stable sort of keys_in whose payload started as every key's index: None when keys_out is
    non-decreasing, payload_out is a permutation, keys_in[payload_out] == keys_out and the payload ascends inside equal
    keys; otherwise a sentence that names the first rule broken."""
    keys_in, keys_out = _u64(keys_in), _u64(keys_out)
    p = np.ascontiguousarray(payload_out).reshape(-1)
    n = keys_in.size
    if keys_out.size != n or p.size != n:
        return "sizes differ"
    if n == 0:
        return None
    if not (keys_out[1:] >= keys_out[:-1]).all():
        return "keys_out descends somewhere"
    if int(p.max()) >= n or int(p.min()) < 0:
        return "payload out of range"
    seen = np.zeros(n, dtype=bool)
    seen[p] = True
    if not seen.all():
        return "payload is not a permutation"
    if not np.array_equal(keys_in[p], keys_out):
        return "a key does not sit with its payload"
    tied = keys_out[1:] == keys_out[:-1]
    if not (p[1:][tied] > p[:-1][tied]).all():
        return "equal keys changed their order"
    return None
