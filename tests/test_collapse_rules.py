"""The rules of collapsing an index by groups (include/sourmash_amd.h, "Collapsing an index by groups") on the plain-Python
restatement alone: hand-written cases against literal set algebra, need_g, and the refusals' conditions.  No device."""
import math

import pytest

import collapse_restatement as CO

A, B, C, D = [1, 2, 3, 4], [3, 4, 5], [4, 5, 6], [9]


def split(offsets, hashes):
    return [hashes[offsets[g]:offsets[g + 1]] for g in range(len(offsets) - 1)]


def test_union_is_the_set_union_of_the_members():
    off, h, ab = CO.collapse([A, B, C, D], [0, 0, 1, 1], 2)
    assert ab is None
    assert split(off, h) == [sorted(set(A) | set(B)), sorted(set(C) | set(D))]
    assert off == [0, 5, 9]


def test_core_is_the_intersection_of_the_members():
    off, h, _ = CO.collapse([A, B, C, D], [0, 0, 0, 1], 2, min_fraction=1.0)
    assert split(off, h) == [sorted(set(A) & set(B) & set(C)), D] == [[4], [9]]


def test_shell_keeps_what_half_of_the_members_hold():
    off, h, _ = CO.collapse([A, B, C], [0, 0, 0], 1, min_fraction=0.5)   # need = ceil(1.5) = 2
    want = sorted(x for x in set(A) | set(B) | set(C) if sum(x in s for s in (A, B, C)) >= 2)
    assert split(off, h) == [want] == [[3, 4, 5]]


def test_min_count_alone_and_with_a_fraction():
    assert split(*CO.collapse([A, B, C], [0, 0, 0], 1, min_count=3)[:2]) == [[4]]
    assert split(*CO.collapse([A, B, C], [0, 0, 0], 1, min_count=2, min_fraction=1.0)[:2]) == [[4]]     # the larger of the two
    assert split(*CO.collapse([A, B, C], [0, 0, 0], 1, min_count=4)[:2]) == [[]]                          # need_g > m_g
    assert split(*CO.collapse([A, B, C], [0, 0, 0], 1, min_count=0)[:2]) == [sorted(set(A) | set(B) | set(C))]   # 0 is read as 1


def test_dropped_nodes_and_empty_groups():
    off, h, _ = CO.collapse([A, B, C, D], [2, None, -1, CO.DROP], 4)
    assert split(off, h) == [[], [], A, []]
    off, h, _ = CO.collapse([A, B], [None, None], 3)
    assert off == [0, 0, 0, 0] and h == []
    assert CO.collapse([], [], 2) == ([0, 0, 0], [], None)
    assert CO.collapse([], [], 2, abund=CO.COUNT) == ([0, 0, 0], [], [])


def test_group_ids_against_node_order():
    off, h, _ = CO.collapse([A, B, C, D], [3, 2, 1, 0], 4)
    assert split(off, h) == [D, C, B, A]
    off, h, _ = CO.collapse([A, B, C, D], [1, 0, 1, 0], 2)
    assert split(off, h) == [sorted(set(B) | set(D)), sorted(set(A) | set(C))]


def test_abundance_modes():
    wa = [(1, 5), (2, 1), (3, 7)]
    wb = [(2, 10), (3, 1), (8, 2)]
    off, h, ab = CO.collapse([wa, wb], [0, 0], 1, abund=CO.SUM)
    assert (h, ab) == ([1, 2, 3, 8], [5, 11, 8, 2])
    off, h, ab = CO.collapse([wa, wb], [0, 0], 1, abund=CO.COUNT)
    assert (h, ab) == ([1, 2, 3, 8], [1, 2, 2, 1])
    off, h, ab = CO.collapse([wa, wb], [0, 0], 1, min_fraction=1.0, abund=CO.SUM)
    assert (h, ab) == ([2, 3], [11, 8])
    assert CO.collapse([wa, wb], [0, 0], 1, abund=CO.FLAT)[2] is None
    assert CO.sketches_of(*CO.collapse([wa, wb], [0, 1], 2, abund=CO.SUM)) == [wa, wb]


def test_hashes_ascend_as_unsigned_64_bit():
    lo, hi = (1 << 63) - 1, 1 << 63
    off, h, _ = CO.collapse([[hi, CO.M64], [0, lo]], [0, 0], 1)
    assert h == [0, lo, hi, CO.M64]


def test_sum_keeps_2_32_minus_1_and_refuses_2_32_naming_the_lowest_group():
    top = (1 << 32) - 1
    off, h, ab = CO.collapse([[(7, top - 1)], [(7, 1)]], [0, 0], 1, abund=CO.SUM)
    assert ab == [top]
    with pytest.raises(CO.Refused, match="group 1 "):
        CO.collapse([[(7, 1)], [(7, top)], [(7, 1)], [(9, top)], [(9, 1)]], [0, 1, 1, 2, 2], 3, abund=CO.SUM)
    # a sum that is not kept is not looked at; COUNT never overflows
    off, h, ab = CO.collapse([[(7, top)], [(7, top)], [(8, 1)]], [0, 0, 0], 1, min_count=3, abund=CO.SUM)
    assert h == []
    assert CO.collapse([[(7, top)], [(7, top)]], [0, 0], 1, abund=CO.COUNT)[2] == [2]


@pytest.mark.parametrize("fraction, want", [
    (0.0, [1, 1, 1, 1, 1, 1, 1]),
    (0.5, [1, 1, 2, 2, 3, 3, 4]),
    (2 / 3, [1, 2, 2, 3, 4, 4, 5]),
    (1.0, [1, 2, 3, 4, 5, 6, 7]),
])
def test_need_for_one_to_seven_members(fraction, want):
    assert [CO.need(m, 1, fraction) for m in range(1, 8)] == want
    assert [CO.need(m, 0, fraction) for m in range(1, 8)] == want
    assert [CO.need(m, 3, fraction) for m in range(1, 8)] == [max(3, w) for w in want]


def test_need_is_the_double_product_not_exact_arithmetic():
    # (2 / 3) * 3 rounds to 2.0 exactly: 3 members need 2; 0.28 * 25 rounds to 7.000000000000001: 25 members need 8, not 7
    assert (2 / 3) * 3 == 2.0 and CO.need(3, 1, 2 / 3) == 2
    assert 0.28 * 25 > 7 and CO.need(25, 1, 0.28) == 8 == math.ceil(0.28 * 25)
    assert CO.need(0, 1, 1.0) == 1 and CO.need(0, 0, 0.0) == 1


def test_argument_refusals():
    for bad in (dict(n_groups=0), dict(min_fraction=-0.01), dict(min_fraction=1.01), dict(min_fraction=float("nan")),
                dict(min_fraction=float("inf")), dict(abund=3)):
        args = dict(n_groups=2, min_fraction=0.5, abund=CO.FLAT)
        args.update(bad)
        with pytest.raises(CO.Refused):
            CO.check_arguments(**args)
    for fine in (0.0, 1.0, 0.5):
        CO.check_arguments(1, fine, CO.COUNT)


def test_group_refusals_name_the_entry():
    with pytest.raises(CO.Refused, match=r"group\[2\] is 5"):
        CO.collapse([A, B, C], [0, 4, 5], 5)
    with pytest.raises(CO.Refused, match=r"group\[0\] is 1"):
        CO.collapse([A], [1], 1)
    assert CO.groups_of([0, None, -1, CO.DROP, 3], 4) == [0, CO.DROP, CO.DROP, CO.DROP, 3]


def test_index_refusals():
    scaled = (0, 21, "DNA", 42, 1 << 60)
    CO.check_index([scaled, scaled], tracks=False, wide=None, abund=CO.COUNT)
    CO.check_index([scaled, scaled], tracks=True, wide=None, abund=CO.SUM)
    CO.check_index([scaled, scaled], tracks=False, wide=0, abund=CO.FLAT)     # abundances are not looked at outside SUM
    CO.check_index([], tracks=True, wide=None, abund=CO.SUM)
    with pytest.raises(CO.Refused, match="node 1 is not a scaled"):
        CO.check_index([scaled, (500, 21, "DNA", 42, 0)], True, None, CO.FLAT)
    with pytest.raises(CO.Refused, match="node 1 is not a scaled"):
        CO.check_index([scaled, (0, 21, "DNA", 42, 0)], True, None, CO.FLAT)
    for other in ((0, 31, "DNA", 42, 1 << 60), (0, 21, "protein", 42, 1 << 60), (0, 21, "DNA", 43, 1 << 60), (0, 21, "DNA", 42, 1 << 59)):
        with pytest.raises(CO.Refused, match="node 2 differs"):
            CO.check_index([scaled, scaled, other], True, None, CO.FLAT)
    with pytest.raises(CO.Refused, match="does not track"):
        CO.check_index([scaled], tracks=False, wide=None, abund=CO.SUM)
    with pytest.raises(CO.Refused, match="node 3 holds an abundance of 2\\^32"):
        CO.check_index([scaled] * 4, tracks=True, wide=3, abund=CO.SUM)
