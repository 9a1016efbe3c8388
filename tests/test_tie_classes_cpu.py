"""The tie-class case lists of tests/tie_classes.py meet their conditions on the CPU oracle, scaling leaves the walk
unchanged, and the oracle agrees with the reference on these cases (tests/golden/tie_classes.json, written by
tests/golden/make_tie_golden.py).

The conditions, per (path kind, traceback word width) list: every target tie class (|S| >= 2) is entered at least 8
times over the list -- a wrong tie-break field agrees with the right one by chance about half the time per visit, so
eight visits leave a miss chance of at most 2^-8 --, every target single-minimum class at least twice, every target
joint class at least once.  Classes that stay short of their count are named in the module with their best count."""
import functools
import json
import os

import pytest

from tests import tie_classes as tc
from tests.conftest import GOLDEN, aln_digest, state_digest

LISTS = [(int8, w) for int8 in (False, True) for w in tc.WIDTHS]
_IDS = [f"{'int8' if i else 'any'}-w{w}" for i, w in LISTS]


@functools.lru_cache(maxsize=None)
def _census(case, k=1):
    return tc.census(tc.scaled_problem(case, k), tc.case_seed(case))


def _summed(cases):
    import collections
    sets, joint = collections.Counter(), collections.Counter()
    for c in cases:
        s, j, _ = _census(c)
        sets.update(s)
        joint.update(j)
    return sets, joint


@pytest.mark.parametrize("int8,width", LISTS, ids=_IDS)
def test_lists_meet_the_conditions(int8, width):
    pairs = tc.width_cases(width, int8)
    assert len(pairs) <= 40
    for case, k in pairs:
        assert max(case[3], case[4]) <= 600
        assert tc.tb_word_bytes(case[2] * k) == width, (case, k)
        if int8:
            assert tc.admissible(tc.scaled_problem(case, k)), (case, k)
    (tset, tjoint), short = tc.targets(width, int8)
    sets, joint = _summed(tc.base_part(pairs))
    lack = tc.deficit(sets, joint, (tset, tjoint))
    # the named exceptions: exactly the classes that stay short, at the counts written down for them
    assert {k[1:]: sets[k[1:]] for k in lack} == short, lack
    assert all(k[0] == "set" for k in lack)


def test_widths_see_both_sides_of_each_switch():
    opens = {w: {c[2] * k for c, k in tc.width_cases(w)} for w in tc.WIDTHS}
    assert {0, 1, 6} <= opens[1] and {7, 126} <= opens[2] and 127 in opens[4]
    assert {c[2] * k for c, k in tc.width_cases(2, True)} >= {7, 126}
    assert {c[2] * k for c, k in tc.width_cases(4, True)} == {127, 130}


def test_zero_list_enters_every_set_class():
    sets, joint = _summed(tc.ZERO)
    assert set(sets) == set(tc.SET_CLASSES)
    # o = 0: no difference lies strictly between 0 and o or equals it without being 0; a joint class is its set class
    assert all(cx in (0, 3) and cy in (0, 3) for _, (_, cx, cy), _ in joint) and len(joint) == 42


def test_scaling_keeps_the_walk():
    """At every factor used: the strings, the random state and the census of the base case, k times its cost."""
    used = sorted({(c, k) for int8, w in LISTS for c, k in tc.width_cases(w, int8) if k != 1})
    assert len({k for _, k in used}) == 11
    for case, k in used:
        s0, j0, ref0 = _census(case)
        s, j, ref = tc.census(tc.scaled_problem(case, k), tc.case_seed(case))
        assert ref[0] == k * ref0[0] and ref[1:] == ref0[1:], (case, k)
        assert s == s0 and j == j0, (case, k)


def test_oracle_matches_the_reference():
    golden = json.load(open(os.path.join(GOLDEN, "tie_classes.json")))
    unscaled = {tuple(g["case"]) for g in golden if g["k"] == 1}
    assert unscaled == set(tc.BASE + tc.ZERO + tc.INT8_LARGE + tc.INT8_126)
    for w in tc.WIDTHS:
        assert sum(g["k"] != 1 and tc.tb_word_bytes(g["case"][2] * g["k"]) == w for g in golden) == 2
    for g in golden:
        case = tuple(g["case"])
        assert g["seed"] == tc.case_seed(case)
        cost, strings, status, words = _census(case, g["k"])[2]
        assert (cost, status, aln_digest(*strings)) == (g["cost"], g["status"], g["aln_sha16"]), case
        assert state_digest((3, words, None)) == g["state_after"], case
