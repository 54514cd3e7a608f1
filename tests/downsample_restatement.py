"""Downsampling restated in plain Python / numpy (the rules of include/sourmash_amd.h, "Downsampling").

No product import: this is what the library's cuts -- on the host, of a sketch in HBM, of a resident index, of a CSR block --
are compared against.

  scaled sketch      num == 0 and max_hash != 0
  max_hash cut       keeps the hashes h <= new (unsigned, inclusive: the comparison add_hash makes, reference
                     src/lib.rs:198) and their abundances; every other parameter is kept; max_hash becomes new
  refused            new == 0; new > max_hash; a sketch that is not scaled
  num cut            keeps the first `new` hashes of a sketch with num != 0 and max_hash == 0; refused for new == 0,
                     new > num and max_hash != 0
  meeting            two scaled operands meet at the smaller max_hash of the two"""
import numpy as np

U64_MAX = (1 << 64) - 1


class Refused(Exception):
    """what the library reports as SOURMASH_ERROR_CODE_MSG (3)"""


def is_scaled(num, max_hash):
    return num == 0 and max_hash != 0


def max_hash_of_scaled(scaled):
    return min((1 << 64) // scaled, U64_MAX)


def scaled_of_max_hash(max_hash):
    return max(1, ((1 << 64) + max_hash // 2) // max_hash)


def cut(mins, abunds, new_max_hash):
    """(mins, abunds) of the ascending `mins` (and the matching `abunds`, or None) that are <= new_max_hash, as Python ints"""
    keep = [i for i, h in enumerate(mins) if int(h) <= int(new_max_hash)]
    assert keep == list(range(len(keep))), "mins must ascend: the cut is a prefix"
    return [int(mins[i]) for i in keep], None if abunds is None else [int(abunds[i]) for i in keep]


def downsample_max_hash(num, max_hash, mins, abunds, new):
    """-> (num, new max_hash, mins, abunds)"""
    if not is_scaled(num, max_hash) or new == 0 or new > max_hash:
        raise Refused((num, max_hash, new))
    m, a = cut(mins, abunds, new)
    return num, new, m, a


def downsample_num(num, max_hash, mins, abunds, new):
    """-> (new num, max_hash, mins, abunds)"""
    if max_hash != 0 or new == 0 or new > num:
        raise Refused((num, max_hash, new))
    return new, max_hash, [int(h) for h in mins[:new]], None if abunds is None else [int(a) for a in abunds[:new]]


def common_max_hash(a_num, a_max_hash, b_num, b_max_hash):
    if not (is_scaled(a_num, a_max_hash) and is_scaled(b_num, b_max_hash)):
        raise Refused((a_num, a_max_hash, b_num, b_max_hash))
    return min(a_max_hash, b_max_hash)


def cut_csr(flat, abunds, offsets, max_hash):
    """The kept prefix of every segment of a CSR (numpy uint64 `flat`, optional uint32 `abunds`, n + 1 `offsets`):
    -> (flat, abunds or None, offsets from 0).  The comparison is made on uint64: unsigned."""
    flat = np.asarray(flat, dtype=np.uint64)
    off = [int(x) for x in offsets]
    mx = np.uint64(max_hash)
    parts, aparts, new_off = [], [], [0]
    for i in range(len(off) - 1):
        seg = flat[off[i]:off[i + 1]]
        k = int(np.searchsorted(seg, mx, side="right"))
        assert np.all(seg[:k] <= mx) and np.all(seg[k:] > mx)
        parts.append(seg[:k])
        if abunds is not None:
            aparts.append(np.asarray(abunds[off[i]:off[i] + k], dtype=np.uint32))
        new_off.append(new_off[-1] + k)
    out = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    out_a = None if abunds is None else (np.concatenate(aparts) if aparts else np.zeros(0, np.uint32))
    return out, out_a, np.array(new_off, dtype=np.uint64)
