"""Collapsing an index by groups restated in plain sequential Python (the rules of include/sourmash_amd.h, "Collapsing an
index by groups").

No product import: this is what the device's child index is compared against, entry for entry.

    sketches      list of n sketches: each a list of hashes, or a list of (hash, abundance) pairs
    group         n entries: the node's group (< n_groups) or DROP / None / -1 for a node that takes no part
    n_groups      G
    min_count     an unsigned 32-bit integer
    min_fraction  a float in [0, 1]
    abund         FLAT, SUM or COUNT

collapse() returns (offsets, hashes, abunds) as ResidentIndex.read() does: G + 1 offsets from 0, the hashes of sketch g
ascending at [offsets[g], offsets[g + 1]), the abundances alongside or None under FLAT."""
import math

FLAT, SUM, COUNT = 0, 1, 2
DROP = 0xFFFFFFFF
M64 = (1 << 64) - 1


class Refused(ValueError):
    """a refusal of the rules (the device call: SOURMASH_ERROR_CODE_MSG)"""


def need(members, min_count, min_fraction):
    """need_g = max(1, min_count, ceil(min_fraction * m_g)): the product and the ceiling in IEEE double"""
    return max(1, min_count, math.ceil(min_fraction * members))


def check_arguments(n_groups, min_fraction, abund):
    """the refusals that need neither the index nor the device"""
    if n_groups == 0:
        raise Refused("n_groups is 0")
    if min_fraction != min_fraction:
        raise Refused("min_fraction is NaN")
    if not 0.0 <= min_fraction <= 1.0:
        raise Refused("min_fraction lies in [0, 1]")
    if abund not in (FLAT, SUM, COUNT):
        raise Refused("unknown abundance mode")


def groups_of(group, n_groups):
    """group[] with None / -1 read as DROP; refuses an entry that is neither below n_groups nor DROP, naming it"""
    out = []
    for v, g in enumerate(group):
        g = DROP if g is None or g == -1 else int(g)
        if g != DROP and g >= n_groups:
            raise Refused("group[%d] is %d; there are %d groups" % (v, g, n_groups))
        out.append(g)
    return out


def check_index(params, tracks, wide, abund):
    """the refusals of the index's nodes.  params: per node (num, ksize, molecule, seed, max_hash); tracks: every node tracks
    abundances that match its hashes; wide: the lowest node holding an abundance of 2^32 or more, or None"""
    for v, p in enumerate(params):
        if not (p[0] == 0 and p[4] != 0):
            raise Refused("node %d is not a scaled sketch" % v)
    for v, p in enumerate(params):
        if p[1:] != params[0][1:]:
            raise Refused("node %d differs from node 0 in ksize, molecule, seed or max_hash" % v)
    if abund == SUM and not tracks:
        raise Refused("the index holds a node that does not track abundances")
    if abund == SUM and wide is not None:
        raise Refused("node %d holds an abundance of 2^32 or more" % wide)


def collapse(sketches, group, n_groups, min_count=1, min_fraction=0.0, abund=FLAT):
    check_arguments(n_groups, min_fraction, abund)
    group = groups_of(group, n_groups)
    if len(group) != len(sketches):
        raise ValueError("one group per node")
    members = [0] * n_groups
    count = [dict() for _ in range(n_groups)]    # c_g(h)
    total = [dict() for _ in range(n_groups)]    # a_g(h)
    for v, sk in enumerate(sketches):
        g = group[v]
        if g == DROP:
            continue
        members[g] += 1
        for item in sk:
            h, a = item if isinstance(item, tuple) else (item, 1)
            count[g][h] = count[g].get(h, 0) + 1
            total[g][h] = total[g].get(h, 0) + a
    offsets, hashes, abunds = [0], [], []
    for g in range(n_groups):
        need_g = need(members[g], min_count, min_fraction)
        kept = sorted(h for h, c in count[g].items() if c >= need_g)   # ascending as unsigned 64-bit: Python ints
        for h in kept:
            if abund == SUM and total[g][h] >= 1 << 32:
                # (groups ascend here, so the first one met is the lowest: the one the message names)
                raise Refused("group %d holds a hash whose abundances add up to 2^32 or more" % g)
        hashes += kept
        abunds += [total[g][h] if abund == SUM else count[g][h] for h in kept]
        offsets.append(len(hashes))
    return offsets, hashes, None if abund == FLAT else abunds


def sketches_of(offsets, hashes, abunds=None):
    """the CSR back as a list of sketches: lists of hashes, or of (hash, abundance) pairs"""
    out = []
    for g in range(len(offsets) - 1):
        a, b = offsets[g], offsets[g + 1]
        out.append(list(zip(hashes[a:b], abunds[a:b])) if abunds is not None else list(hashes[a:b]))
    return out
