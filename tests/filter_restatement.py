"""Filtering a resident index and taking a subset of its nodes, restated in plain Python over lists from the rules of
include/sourmash_amd.h ("Filtering an index") -- not from the C++.  Every result is an integer: the device must be EQUAL.

A sketch is a list of hashes, or of (hash, abundance) pairs; an index is a list of sketches and has abundances when
`has_abunds` says so (default: when its elements are pairs).  The operand is such a list too, or None.

  filter(sketches, operand, rule)  -> (offsets, hashes, abunds | None)
  select(sketches, ids)            -> (offsets, hashes, abunds | None)

Refusals raise Refused(code, message): code 3 and a message that begins with "filter:" (or "select:"), except an operand that
is incompatible with the nodes, whose code (101-104) the caller states."""
import collections

NONE, KEEP_IN, DROP_IN = 0, 1, 2
OWN, FLAT, OPERAND = 0, 1, 2
NO_MAX = 0xFFFFFFFF
MSG = 3

Rule = collections.namedtuple("Rule", ["operand_mode", "abund_out", "min_abund", "max_abund", "min_owners", "max_owners"])
Rule.__new__.__defaults__ = (NONE, OWN, 0, NO_MAX, 0, NO_MAX)


class Refused(Exception):
    def __init__(self, code, message):
        super().__init__(message)
        self.code, self.message = code, message


def _refuse(what):
    raise Refused(MSG, "filter: " + what)


def _pairs(sketch):
    """(hash, abundance or None) of every element, ascending by hash"""
    return sorted((x if isinstance(x, tuple) else (x, None)) for x in sketch)


def _weighted(sketches):
    elems = [x for s in sketches for x in s]
    return bool(elems) and all(isinstance(x, tuple) for x in elems)


def abund_window(rule):
    return not (rule.min_abund == 0 and rule.max_abund == NO_MAX)


def owner_window(rule):
    return not (rule.min_owners <= 1 and rule.max_owners == NO_MAX)


def filter(sketches, operand, rule, has_abunds=None, operand_tracks=None, node_scaled=None, operand_scaled=True, incompatible=0,
           directory_limit=1 << 31, have_index=True):
    """node_scaled: one bool per node (default: all scaled); incompatible: the code check_compatible gives the operand, 0: none"""
    # --- the refusals, in the header's order; nothing is built before the last of them
    if rule is None:
        _refuse("rule is NULL")
    if rule.operand_mode not in (NONE, KEEP_IN, DROP_IN):
        _refuse("unknown operand mode %d" % rule.operand_mode)
    if rule.abund_out not in (OWN, FLAT, OPERAND):
        _refuse("unknown abundance mode %d" % rule.abund_out)
    if rule.min_abund > rule.max_abund:
        _refuse("min_abund %d exceeds max_abund %d" % (rule.min_abund, rule.max_abund))
    if rule.min_owners > rule.max_owners:
        _refuse("min_owners %d exceeds max_owners %d" % (rule.min_owners, rule.max_owners))
    if rule.abund_out == OPERAND and rule.operand_mode != KEEP_IN:
        _refuse("the operand's abundances can be given only to the hashes kept in it")
    if not have_index:
        _refuse("index is NULL")
    if has_abunds is None:
        has_abunds = _weighted(sketches)
    for i, ok in enumerate(node_scaled or ()):
        if not ok:
            _refuse("node %d is not a scaled sketch" % i)
    if rule.operand_mode != NONE:
        if operand is None:
            _refuse("operand is NULL")
        if not operand_scaled:
            _refuse("the operand is not a scaled sketch")
        if incompatible:
            raise Refused(incompatible, "mismatch")
        if operand_tracks is None:
            operand_tracks = _weighted([operand])
        if rule.abund_out == OPERAND and not operand_tracks:
            _refuse("the operand does not track abundances")
    if abund_window(rule) and not has_abunds:
        _refuse("an abundance window on an index that holds a node that does not track abundances")
    if abund_window(rule) or (rule.abund_out == OWN and has_abunds):
        for i, s in enumerate(sketches):
            if any(a is not None and a >> 32 for _, a in _pairs(s)):
                _refuse("node %d holds an abundance of 2^32 or more" % i)
    if rule.abund_out == OPERAND and any(a is not None and a >> 32 for _, a in _pairs(operand)):
        _refuse("the operand holds an abundance of 2^32 or more")
    if owner_window(rule) and sum(len(s) for s in sketches) >= directory_limit:
        _refuse("the index holds %d hashes; the directory takes fewer than 2^31" % sum(len(s) for s in sketches))

    # --- the rule: three conditions, each judged on the parent
    op = dict(_pairs(operand)) if rule.operand_mode != NONE else {}
    owners = collections.Counter(h for s in sketches for h, _ in _pairs(s))
    child_abunds = rule.abund_out == OPERAND or (rule.abund_out == OWN and has_abunds)
    offsets, hashes, abunds = [0], [], []
    for s in sketches:
        for h, a in _pairs(s):
            if rule.operand_mode == KEEP_IN and h not in op:
                continue
            if rule.operand_mode == DROP_IN and h in op:
                continue
            if abund_window(rule) and not rule.min_abund <= a <= rule.max_abund:
                continue
            if not rule.min_owners <= owners[h] <= rule.max_owners:
                continue
            hashes.append(h)
            abunds.append(op[h] if rule.abund_out == OPERAND else a)
        offsets.append(len(hashes))
    return offsets, hashes, abunds if child_abunds else None


def select(sketches, ids, has_abunds=None):
    n = len(sketches)
    for j, v in enumerate(ids):
        if v >= n:
            raise Refused(MSG, "select: ids[%d] is %d; the index has %d nodes" % (j, v, n))
    if has_abunds is None:
        has_abunds = _weighted(sketches)
    offsets, hashes, abunds = [0], [], []
    for v in ids:
        for h, a in _pairs(sketches[v]):
            hashes.append(h)
            abunds.append(a)
        offsets.append(len(hashes))
    return offsets, hashes, abunds if has_abunds else None
