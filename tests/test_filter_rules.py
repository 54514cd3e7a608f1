"""The rules of filtering a resident index (include/sourmash_amd.h, "Filtering an index") on hand-worked cases through the
plain-Python restatement, the constants of the header, and the restatement's refusals against the header's list.  No GPU."""
import os
import re

import pytest

import filter_restatement as F
from conftest import ROOT

R = F.Rule

# node 0 {1, 2, 3, 4}, node 1 {3, 4, 5}, node 2 {5, 6}, node 3 {}: owners 1:1 2:1 3:2 4:2 5:2 6:1; abundances = 10 * hash + node
SK = [[(1, 10), (2, 20), (3, 30), (4, 40)], [(3, 31), (4, 41), (5, 51)], [(5, 52), (6, 62)], []]
FLAT = [[h for h, _ in s] for s in SK]
OP = [(2, 7), (3, 8), (5, 9), (99, 1)]


def test_operand_modes():
    assert F.filter(FLAT, [2, 3, 5, 99], R(F.KEEP_IN)) == ([0, 2, 4, 5, 5], [2, 3, 3, 5, 5], None)
    assert F.filter(FLAT, [2, 3, 5, 99], R(F.DROP_IN)) == ([0, 2, 3, 4, 4], [1, 4, 4, 6], None)
    assert F.filter(FLAT, None, R()) == ([0, 4, 7, 9, 9], [1, 2, 3, 4, 3, 4, 5, 5, 6], None)
    # the two modes are complementary; an empty operand keeps nothing / everything
    assert F.filter(FLAT, [], R(F.KEEP_IN)) == ([0, 0, 0, 0, 0], [], None)
    assert F.filter(FLAT, [], R(F.DROP_IN))[1] == F.filter(FLAT, None, R())[1]


def test_abundances_of_the_child():
    assert F.filter(SK, OP, R(F.KEEP_IN)) == ([0, 2, 4, 5, 5], [2, 3, 3, 5, 5], [20, 30, 31, 51, 52])
    assert F.filter(SK, OP, R(F.KEEP_IN, F.FLAT)) == ([0, 2, 4, 5, 5], [2, 3, 3, 5, 5], None)
    assert F.filter(SK, OP, R(F.KEEP_IN, F.OPERAND)) == ([0, 2, 4, 5, 5], [2, 3, 3, 5, 5], [7, 8, 8, 9, 9])
    # inflate gives flat nodes the operand's abundances
    assert F.filter(FLAT, OP, R(F.KEEP_IN, F.OPERAND)) == ([0, 2, 4, 5, 5], [2, 3, 3, 5, 5], [7, 8, 8, 9, 9])
    assert F.filter(SK, None, R(abund_out=F.FLAT)) == ([0, 4, 7, 9, 9], [1, 2, 3, 4, 3, 4, 5, 5, 6], None)


def test_abundance_window_edges():
    # both ends belong to the window
    assert F.filter(SK, None, R(min_abund=30, max_abund=41)) == ([0, 2, 4, 4, 4], [3, 4, 3, 4], [30, 40, 31, 41])
    assert F.filter(SK, None, R(min_abund=31, max_abund=40)) == ([0, 1, 2, 2, 2], [4, 3], [40, 31])
    assert F.filter(SK, None, R(min_abund=62)) == ([0, 0, 0, 1, 1], [6], [62])
    assert F.filter(SK, None, R(max_abund=10)) == ([0, 1, 1, 1, 1], [1], [10])
    assert F.filter([[(1, 1), (2, 2)], [(2, 1)]], None, R(min_abund=1, max_abund=1)) == ([0, 1, 2], [1, 2], [1, 1])
    # the window reads the node's OWN abundance even when the child takes the operand's
    assert F.filter(SK, OP, R(F.KEEP_IN, F.OPERAND, min_abund=31)) == ([0, 0, 2, 3, 3], [3, 5, 5], [8, 9, 9])


def test_owner_window_edges():
    assert F.filter(FLAT, None, R(max_owners=1)) == ([0, 2, 2, 3, 3], [1, 2, 6], None)
    assert F.filter(FLAT, None, R(min_owners=2)) == ([0, 2, 5, 6, 6], [3, 4, 3, 4, 5, 5], None)
    assert F.filter(FLAT, None, R(min_owners=1, max_owners=1)) == F.filter(FLAT, None, R(max_owners=1))
    assert F.filter(FLAT, None, R(min_owners=3, max_owners=3)) == ([0, 0, 0, 0, 0], [], None)
    assert not F.owner_window(R(min_owners=1)) and not F.owner_window(R()) and F.owner_window(R(min_owners=2))
    assert F.owner_window(R(max_owners=F.NO_MAX - 1)) and not F.abund_window(R()) and F.abund_window(R(min_abund=1))


def test_the_conjunction_is_evaluated_on_the_parent():
    # owners(h) counts the PARENT's nodes: a hash the operand or the abundance window removes from one node still counts as
    # held by it.  4 is dropped from no node and 3 from both, yet neither becomes private to anyone.
    assert F.filter(SK, [3], R(F.DROP_IN, max_owners=1)) == ([0, 2, 2, 3, 3], [1, 2, 6], [10, 20, 62])
    assert F.filter(SK, None, R(min_abund=41, max_owners=1)) == ([0, 0, 0, 1, 1], [6], [62])
    assert F.filter(SK, None, R(min_abund=41, min_owners=2)) == ([0, 0, 2, 3, 3], [4, 5, 5], [41, 51, 52])


def test_select():
    assert F.select(SK, [2, 0, 2, 3]) == ([0, 2, 6, 8, 8], [5, 6, 1, 2, 3, 4, 5, 6], [52, 62, 10, 20, 30, 40, 52, 62])
    assert F.select(FLAT, []) == ([0], [], None)
    assert F.select(FLAT, [1]) == ([0, 3], [3, 4, 5], None)
    with pytest.raises(F.Refused) as ei:
        F.select(FLAT, [0, 4])
    assert ei.value.code == 3 and ei.value.message.startswith("select: ids[1] is 4")


def test_refusals_mirror_the_header():
    wide = [[(1, 1)], [(2, 1 << 32)]]
    cases = [
        (dict(rule=None), "rule is NULL"),
        (dict(rule=R(3)), "unknown operand mode 3"),
        (dict(rule=R(abund_out=3)), "unknown abundance mode 3"),
        (dict(rule=R(min_abund=2, max_abund=1), sketches=SK), "min_abund 2 exceeds max_abund 1"),
        (dict(rule=R(min_owners=5, max_owners=4)), "min_owners 5 exceeds max_owners 4"),
        (dict(rule=R(F.DROP_IN, F.OPERAND), operand=OP), "only to the hashes kept in it"),
        (dict(rule=R(F.NONE, F.OPERAND)), "only to the hashes kept in it"),
        (dict(rule=R(), have_index=False), "index is NULL"),
        (dict(rule=R(), node_scaled=[True, False, True, True]), "node 1 is not a scaled sketch"),
        (dict(rule=R(F.KEEP_IN), operand=None), "operand is NULL"),
        (dict(rule=R(F.DROP_IN), operand=[1], operand_scaled=False), "the operand is not a scaled sketch"),
        (dict(rule=R(F.KEEP_IN, F.OPERAND), operand=[1, 2]), "the operand does not track abundances"),
        (dict(rule=R(min_abund=1)), "an abundance window on an index"),
        (dict(rule=R(), sketches=wide), "node 1 holds an abundance of 2^32 or more"),
        (dict(rule=R(max_abund=5), sketches=wide), "node 1 holds an abundance of 2^32 or more"),
        (dict(rule=R(F.KEEP_IN, F.OPERAND), operand=[(1, 1 << 32)]), "the operand holds an abundance of 2^32 or more"),
        (dict(rule=R(max_owners=1), directory_limit=9), "the directory takes fewer than 2^31"),
    ]
    for kw, words in cases:
        kw.setdefault("sketches", FLAT)
        kw.setdefault("operand", None)
        with pytest.raises(F.Refused) as ei:
            F.filter(**kw)
        assert ei.value.code == F.MSG and ei.value.message.startswith("filter: ") and words in ei.value.message, words
    with pytest.raises(F.Refused) as ei:
        F.filter(FLAT, [1], R(F.KEEP_IN), incompatible=102)
    assert ei.value.code == 102
    # what abundances refuse, a rule that does not involve them takes: FLAT on the wide index, no window
    assert F.filter(wide, None, R(abund_out=F.FLAT)) == ([0, 1, 2], [1, 2], None)
    assert F.filter(wide, [(2, 5)], R(F.KEEP_IN, F.OPERAND)) == ([0, 0, 1], [2], [5])
    # these are no refusals: an empty index, empty nodes, an empty operand, a rule that keeps nothing
    assert F.filter([], None, R(max_owners=1)) == ([0], [], None)
    assert F.filter([[], []], [], R(F.KEEP_IN, F.OPERAND, max_owners=1), operand_tracks=True) == ([0, 0, 0], [], [])
    assert F.filter(FLAT, None, R(min_owners=4)) == ([0, 0, 0, 0, 0], [], None)


def test_header_states_the_rules():
    header = open(os.path.join(ROOT, "include", "sourmash_amd.h")).read()
    assert "enum { SMH_FILTER_OPERAND_NONE = 0, SMH_FILTER_KEEP_IN = 1, SMH_FILTER_DROP_IN = 2 };" in header
    assert "enum { SMH_FILTER_ABUND_OWN = 0, SMH_FILTER_ABUND_FLAT = 1, SMH_FILTER_ABUND_OPERAND = 2 };" in header
    assert (F.NONE, F.KEEP_IN, F.DROP_IN, F.OWN, F.FLAT, F.OPERAND) == (0, 1, 2, 0, 1, 2)
    struct = re.search(r"typedef struct SmhFilter \{(.*?)\} SmhFilter;", header, flags=re.S)
    assert struct is not None
    fields = re.findall(r"\b(operand_mode|abund_out|min_abund|max_abund|min_owners|max_owners)\b", re.sub(r"/\*.*?\*/", "", struct.group(1)))
    assert tuple(fields) == F.Rule._fields
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "SmhIndex *smh_index_filter(SmhIndex *index, const KmerMinHash *operand, const SmhFilter *rule);" in code
    assert "SmhIndex *smh_index_select(SmhIndex *index, const uint32_t *ids, uint32_t n_ids);" in code
    assert "void smh_filter_geometry(uint32_t *tile, uint32_t *operand_samples, uint32_t *threads);" in code
    assert '"filter_flag"' in header and '"filter_emit"' in header and '"index_filtered"' in header and '"index_selected"' in header
