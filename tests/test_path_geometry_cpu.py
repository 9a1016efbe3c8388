"""The path-geometry case lists of tests/path_geometry.py meet their conditions on the CPU oracle at every traceback
word width, stay within their size and count caps, and the oracle agrees with the reference on them
(tests/golden/path_geometry.json, written by tests/golden/make_path_golden.py).

The conditions W1-W8 (path_geometry.REQUIRED names the code each guards) count a class only when at least two
different cases reach it, unless it is asked for once or as a sum over the list.  No class is left short: the int8
paths' four-byte lists, which the "gap" table (sub' = 2 o + 2) leaves, take the "gap8" table (sub' = 125) for their
Z corners."""
import functools
import json
import os

import pytest

from tests import path_geometry as pg
from tests.conftest import GOLDEN, aln_digest, state_digest

LISTS = [(path, w, False) for path in pg.PATHS for w in pg.WIDTHS] + \
        [(path, w, True) for path in ("single", "rc", "pipe") for w in pg.WIDTHS]
_IDS = [f"{p}-w{w}{'-int8' if i else ''}" for p, w, i in LISTS]


@functools.lru_cache(maxsize=None)
def _census(case):
    return pg.census(pg.problem(case), pg.case_seed(case))


def _lack(cases, groups):
    return pg.deficit(cases, groups, {c: _census(c) for c in cases})


@pytest.mark.parametrize("path,width,int8", LISTS, ids=_IDS)
def test_lists_meet_the_conditions(path, width, int8):
    cases = pg.path_cases(path, width, int8)
    names, groups = pg.PATHS[path]
    assert len(set(cases)) == len(cases)
    for name in names:
        assert len(pg.LISTS[name]) <= pg.COUNT_CAP, name
    for case in cases:
        m, n = pg.shape(case)
        prob = pg.problem(case)
        assert (len(prob[1]), len(prob[2])) == (m, n)
        assert max(m, n) <= pg.SIDE_CAP and (m + 1) * (n + 1) <= pg.CELL_CAP, case
        assert pg.tb_word_bytes(case[0][1]) == width, case
        if int8:
            assert pg.admissible(prob), case
        if path == "rc":
            assert min(m, n) >= 256, case
        if path == "batch":
            assert m * n <= pg.BATCH_CELL_CAP, case
        # every case's oracle status is "ok"
        assert _census(case).ref[2] == "ok", case
    # the named exceptions: exactly the classes that stay short
    assert _lack(cases, groups) == pg.short(path, width, int8)


def test_no_list_is_short_and_int8_lists_keep_their_gap_moves():
    assert not [k for k in LISTS if pg.short(*k)]
    # at four-byte words the int8 lists hold the same entries as the others, the "gap" table replaced by "gap8"
    wide, int8 = pg.path_cases("single", 4), pg.path_cases("single", 4, True)
    assert [c[1:] for c in wide] == [c[1:] for c in int8]
    assert {(a[0], b[0]) for a, b in zip(wide, int8) if a != b} == {(("gap", 127), ("gap8", 127))}
    # ... under which the walk still reaches row 0 by a level-2 move and column 0 by a level-1 move, in every
    # distance class
    gap_moves = {_census(c).arrival[:2] + (pg._dist_class(_census(c).arrival[2]),) for c in int8 if c[0][0] == "gap8"
                 and _census(c).arrival[0] != "corner"}
    assert gap_moves == {(e, L, k) for e, L in (("row", 2), ("col", 1)) for k in range(len(pg.DIST_CLASSES))}
    for w in (1, 2):
        assert pg.path_cases("single", w) == pg.path_cases("single", w, True)


def test_widths_take_their_gap_open_costs():
    opens = {w: {c[0] for c in pg.path_cases("single", w)} for w in pg.WIDTHS}
    assert opens[1] == {("dna", 5), ("gap", 3), ("gap", 0)}
    assert opens[2] == {("dna", 7), ("dna", 8), ("dna", 9), ("gap", 8)}
    assert opens[4] == {("dna", 127), ("dna", 130), ("gap", 127)}


def test_a_needed_case_cannot_be_removed():
    """The conditions notice a missing case: without its D = 2048 entry the COUNT list lacks the ring-wrap class, and
    with only one of the level-2 arrivals on row 0 at 17..24 columns left the lists lack that class."""
    cases = pg.path_cases("single", 1)
    without = [c for c in cases if _census(c).D != 2048]
    assert len(without) == len(cases) - 1
    assert _lack(without, ("W6",)) == {("W6", "D", 2048): 1}
    hit = [c for c in cases if _census(c).arrival[:2] == ("row", 2) and 17 <= _census(c).arrival[2] <= 24]
    assert len(hit) >= 2
    assert _lack([c for c in cases if c not in hit[1:]], ("W4",)) == {("W4", "row", 2, 1): 1}


def test_slab_edges_restated():
    from globalign_amd import distributed
    for case in pg.path_cases("slabs", 1):
        n = pg.shape(case)[1]
        assert pg.slab_bounds(n) == distributed.slab_bounds(n, 3)
        assert pg.slab_bounds(n)[1:3] == [512, 1024]


def test_oracle_matches_the_reference():
    golden = json.load(open(os.path.join(GOLDEN, "path_geometry.json")))

    def key(rec):
        (kind, o), segments, seed = rec["case"]
        return ((kind, o), tuple(tuple(s) for s in segments), seed)
    assert [key(g) for g in golden] == pg.golden_cases()
    # every entry under 4 * 10^5 cells is there, and at least one case of every list (so of every group W1-W8)
    small = {c for path in pg.PATHS for c in pg.path_cases(path, 1)
             if (pg.shape(c)[0] + 1) * (pg.shape(c)[1] + 1) < pg.GOLDEN_CELLS}
    have = {key(g) for g in golden}
    assert small <= have
    for name, bases in pg.LISTS.items():
        assert pg.at_width(bases[0], 1, 0) in have, name
    assert {pg.tb_word_bytes(k[0][1]) for k in have} == set(pg.WIDTHS)
    for g in golden:
        case = key(g)
        assert g["seed"] == pg.case_seed(case)
        cost, strings, status, words = _census(case).ref
        assert (cost, status, aln_digest(*strings)) == (g["cost"], g["status"], g["aln_sha16"]), case
        assert state_digest((3, words, None)) == g["state_after"], case
