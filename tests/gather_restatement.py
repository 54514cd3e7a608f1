"""Gather restated in plain Python over sets (the rules of include/sourmash_amd.h, smh_index_gather).

No product import: this is what the device kernels are compared against, value for value.

    sketches   list of iterables of hashes (S_0 .. S_{n-1})
    query      iterable of hashes; position p = the p-th hash in ascending order
    abunds     {hash: abundance} of the query, or None (every hash weighs 1)
    threshold  threshold_common; 0 is read as 1
    capacity   row capacity

Returns (rows, assigned): rows as dicts with the integers of SmhGatherRow, assigned[p] = the round that consumed position
p or UNASSIGNED."""
import math

UNASSIGNED = 0xFFFFFFFF


def gather(sketches, query, abunds=None, threshold=0, capacity=None):
    sets = [set(s) for s in sketches]
    q_sorted = sorted(set(query))
    pos = {h: p for p, h in enumerate(q_sorted)}
    full = set(q_sorted)
    threshold = max(1, threshold)
    if capacity is None:
        capacity = len(sets)
    remaining = set(q_sorted)
    assigned = [UNASSIGNED] * len(q_sorted)
    rows = []
    alive = list(range(len(sets)))   # `remaining` only shrinks: a sketch whose count reached 0 stays there and is not recounted
    while True:
        r = len(rows)
        best, c_best = 0, 0
        counts = [(i, len(remaining & sets[i])) for i in alive]
        alive = [i for i, c in counts if c > 0]
        for i, c in counts:
            if c > c_best:          # strictly more: the lowest index keeps a tie
                best, c_best = i, c
        if c_best < threshold or r == capacity:
            break
        took = remaining & sets[best]
        rows.append({"match": best, "common_remaining": c_best, "common_original": len(full & sets[best]),
                     "size_match": len(sets[best]),
                     "abund_sum": sum(abunds[h] for h in took) if abunds is not None else len(took)})
        for h in took:
            assigned[pos[h]] = r
        remaining -= took
    return rows, assigned


def cut(rows, assigned, capacity):
    """gather(..., capacity=capacity) from the result of a run without a capacity: the capacity only ends the loop early, so
    the rows are a prefix and the positions later rounds consumed stay unassigned (test_gather_rules checks this identity
    against gather() itself).  Lets one full run of a large case serve every capacity."""
    return rows[:capacity], [a if a < capacity else UNASSIGNED for a in assigned]


def ties(sketches, query, threshold=0, capacity=None):
    """the rounds in which a sketch other than the winner had the winning count (decided by the lowest-index rule)"""
    sets = [set(s) for s in sketches]
    rows, _ = gather(sketches, query, None, threshold, capacity)
    remaining = set(query)
    out = []
    for r, row in enumerate(rows):
        if sum(1 for s in sets if len(remaining & s) == row["common_remaining"]) > 1:
            out.append(r)
        remaining -= sets[row["match"]]
    return out


def derived(rows, assigned, n_query, q_abunds, scaled):
    """The floats the Python wrapper derives from the integers, by the same formulas: q_abunds = the query's abundances in
    position order (None: 1 each).  median / std are left to the caller (numpy over assigned)."""
    total = sum(q_abunds) if q_abunds is not None else n_query
    out, left = [], n_query
    for row in rows:
        left -= row["common_remaining"]
        out.append({"f_orig_query": row["common_original"] / n_query,
                    "f_match": row["common_remaining"] / row["size_match"],
                    "f_unique_to_query": row["common_remaining"] / n_query,
                    "f_unique_weighted": row["abund_sum"] / total,
                    "average_abund": row["abund_sum"] / row["common_remaining"],
                    "remaining_bp": scaled * left})
    return out


def threshold_common(threshold_bp, scaled):
    return int(math.ceil(threshold_bp / scaled))
