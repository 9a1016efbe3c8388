"""CPU checks of tests/limit_costs.py: the cases the GPU limit tests run can fail, reach the magnitudes they are meant
to reach and sit exactly on the restated guard; the oracle is pinned against the reference at these magnitudes
(tests/golden/limit_costs.json, written by tests/golden/make_limit_golden.py)."""
import collections
import functools
import json
import math
import os
import random

import numpy as np
import pytest

from oracle import core
from tests import general_costs as gc
from tests import limit_costs as lc
from tests.conftest import GOLDEN, state_digest


_V_BATCHES = ((lc.V16, lc.V_BATCH_SHAPES), (lc.VPHI, lc.V_BATCH_SHAPES), (lc.VNEG, lc.V_BATCH_SHAPES),
              (lc.V32, lc.V32_SHAPES))


def _family_group(case):
    return "K" if case[0][0] == "K" else case[0]


@functools.lru_cache(maxsize=None)
def _cost(case):
    cmat, s1, s2, o = lc.problem(case)
    return gc.oracle_cost(cmat, s1, s2, o)


def test_limit_cases_can_fail():
    """Every eligible single-call and batch case: the oracle's cost changes under each corruption of what a kernel
    reads for the case's family -- an int8 entry zero-extended, an int16 entry cut to its low byte or zero-extended, a
    4-byte entry cut to int16, a letter code cut to five bits, the last letter's code off by one."""
    cases = lc.all_single_cases()
    for fam in (lc.P8, lc.P8A, lc.P16, lc.P16A, lc.P16B):
        cases += lc.batch_cases(fam, lc.BATCH_COST_SHAPES, 20)
    for fam in (lc.K_(64, 600), lc.K_(65, 600), lc.K_(90, 5), lc.K_(91, 5), lc.K_(128), lc.K_(129), lc.K_(255)):
        cases += lc.batch_cases(fam, lc.K_BATCH_SHAPES, 20)
    met, kinds = collections.Counter(), collections.Counter()
    for case in dict.fromkeys(cases):
        if not lc.eligible(case):
            continue
        base = _cost(case)
        todo = lc.corruptions(case)
        assert todo, case
        for what, kind in todo:
            assert lc.corrupted_cost(case, what, kind) != base, (case, what, kind)
            kinds[kind] += 1
        met[_family_group(case)] += 1
    # the V families' batches: every pair under the batch's one table (the largest pair's factor)
    for fam, shapes in _V_BATCHES:
        cmat, batch, _ = lc.v_batch_cases(fam, shapes, lc.O_MAX)
        todo = lc.table_corruptions(cmat)
        for case in batch:
            if not lc.eligible(case):
                continue
            s1, s2 = lc.sequences(case)
            base = gc.oracle_cost(cmat, s1, s2, lc.O_MAX)
            for _, kind in todo:
                assert gc.oracle_cost(lc.corrupt_table(cmat, kind), s1, s2, lc.O_MAX) != base, (case, kind)
                kinds[kind] += 1
            met[fam[0] + " batch"] += 1
    print("limit cases that can fail under every corruption:", dict(met), dict(kinds))
    assert set(kinds) == set(lc.TABLE_CORRUPTIONS) | {"low5", "last"}
    assert dict(met) == EXPECTED_CAN_FAIL


# every eligible case of the lists, none dropped unnoticed (K: the Kn families together)
EXPECTED_CAN_FAIL = {"P8": 22, "P8+a": 16, "P8+b": 5, "P16": 15, "P16+a": 7, "P16+b": 7, "K": 63, "V16": 5, "Vphi": 17,
                     "V-": 6, "V16 batch": 7, "Vphi batch": 7, "V- batch": 7, "V32 batch": 2}


def _reach(case, custom):
    """max |stored value| over every cell and level, plain and shifted by GV(i) + GH(j)."""
    cmat, s1, s2, o = lc.problem(case)
    tab = core.Tables(cmat)
    a, b = tab.codes(s1), tab.codes(s2)
    m, n = len(a), len(b)
    if custom:
        row0, col0 = (np.array(x, dtype=np.int64) for x in lc.vb_boundary(case))
    else:
        row0, col0 = core.boundary(tab, a, b, o, (tab.max_cost + 1) * max(m, n))
    dp = np.zeros((m + 1, n + 1, 3), np.int64)
    dp[0, :, :] = row0.reshape(n + 1, 3)
    dp[:, 0, :] = col0.reshape(m + 1, 3)
    core.fill_full(tab, a, b, o, dp)
    GV = np.concatenate([[0], np.cumsum(tab.gv[a])])
    GH = np.concatenate([[0], np.cumsum(tab.gh[b])])
    shifted = dp - GV[:, None, None] - GH[None, :, None]
    return int(np.abs(dp).max()), int(np.abs(shifted).max())


def _v_cases():
    cases = [c for c in lc.all_single_cases() if lc.is_v(c)]
    for fam, shapes in ((lc.V16, lc.V_BATCH_SHAPES), (lc.VPHI, lc.V_BATCH_SHAPES), (lc.V32, lc.V32_SHAPES)):
        cmat, batch, f = lc.v_batch_cases(fam, shapes, lc.O_MAX)
        # a batch runs under one table: its largest pair is the one that has to reach 2^25
        cases.append(max(batch, key=lambda c: c[2] + c[3]))
    return list(dict.fromkeys(cases))


def test_limit_cases_reach_2_25():
    """Above 2^24 a value no longer survives a round trip through fp32 or a 24-bit operand: every V case, and every
    case under a near-guard caller boundary, stores a value of at least 2^25 (a condition on the inputs)."""
    worst, worst_shifted = {}, {}
    for custom, cases in ((False, _v_cases()), (True, lc.all_custom_cases())):
        for case in cases:
            plain, shifted = _reach(case, custom)
            got = max(plain, shifted)
            assert got >= 2 ** 25, (case, math.log2(got))
            assert 4 * got < 2 ** 31, case  # and what the guard promises holds
            worst[case[0]] = min(worst.get(case[0], 99.0), math.log2(got))
            worst_shifted[case[0]] = min(worst_shifted.get(case[0], 99.0), math.log2(shifted))
    print("least log2(max |stored value|) per family:", {k: round(v, 2) for k, v in worst.items()})
    # (the kernels compute in the shifted domain: under Vphi / V- its interior is small by construction, the
    # magnitude is in row 0 / column 0, big and the un-shift; V16 / V32 / VB carry it through every cell)
    print("  of that, shifted by GV(i) + GH(j):", {k: round(v, 2) for k, v in worst_shifted.items()})
    assert set(worst) == {"V16", "V32", "Vphi", "V-", "VB+", "VB-"}


def test_v_factor_sits_on_the_guard():
    """The chosen factor of every V case passes the restated checks, factor + 1 fails them; the VB bound likewise."""
    for case in _v_cases():
        family, _, m, n, o = case
        ok = lc.batch_accepts if family == "V32" else lc.single_accepts
        assert ok(lc.v_table(family, m, n, o), m, n, o) and not ok(lc.v_table(family, m, n, o, excess=1), m, n, o), case
    for case in lc.all_custom_cases():
        B = lc.vb_bound(case)
        row0, col0 = lc.vb_boundary(case)
        big = max(abs(v) for v in row0 + col0)
        assert big == B and B > 2 ** 28.9, (case, B)
    # the figures ga_host_selftest.cpp checks check_problem against
    assert lc.v_factor("V16", 1100, 600, lc.O_MAX) == 6553
    assert lc.v_factor("V16", 4096, 1024, 5) == PINNED["V16 4096x1024"]
    assert lc.v_factor("Vphi", 777, 2049, 7) == PINNED["Vphi 777x2049"]
    assert lc.v_factor("V-", 2049, 700, 5) == PINNED["V- 2049x700"]
    assert lc.v_factor("V32", 65, 70, lc.O_MAX) == PINNED["V32 65x70"]


PINNED = {"V16 4096x1024": 5516, "Vphi 777x2049": 25415, "V- 2049x700": 32462, "V32 65x70": 221364}


def test_widths_restated():
    assert [lc.tb_word_bytes(o) for o in (6, 7, 126, 127, 32766, 32767)] == [1, 2, 2, 4, 4, 0]
    assert [lc.profile_bytes(lc.p_table(f)) for f in ("P8", "P8+a", "P8+b", "P16", "P16+a", "P16+b")] == [1, 2, 2, 2, 0, 0]
    for K in (32, 33, 64, 65, 90, 91, 128, 129, 255):
        for case in (lc.K_(K) + (K + 90, K + 100, 6), lc.K_(K) + (3, 70, 6)):
            s1, s2 = lc.sequences(case)
            last = lc.k_keys(K)[K - 2]
            assert last in s1 and last in s2 and (len(s1), len(s2)) == case[2:4]
            if case[2] > K:
                assert lc.all_codes_occur(s1, K) and lc.all_codes_occur(s2, K), case
                # the highest codes on both sides of position 64
                top = set(lc.k_keys(K)[K - 9:K - 1])
                assert set(s1[60:64]) <= top and set(s1[64:68]) <= top and set(s2[60:68]) <= top
        assert len(set(lc.k_keys(K))) == K and all(len(k) == 1 for k in lc.k_keys(K))


def _walk_with_fields(problem, seed, saturate_at):
    """The oracle's full-array walk over cells rebuilt from a traceback word's fields: X and Y of every
    interior cell become H + min(X - H, saturate_at) and H + min(Y - H, saturate_at).  -> (status, strings)"""
    import ctypes as C
    cmat, s1, s2, o = problem
    tab = core.Tables(cmat)
    a, b = tab.codes(s1), tab.codes(s2)
    m, n = len(a), len(b)
    row0, col0 = core.boundary(tab, a, b, o, (tab.max_cost + 1) * max(m, n))
    dp = np.zeros((m + 1, n + 1, 3), np.int64)
    dp[0, :, :] = row0.reshape(n + 1, 3)
    dp[:, 0, :] = col0.reshape(m + 1, 3)
    core.fill_full(tab, a, b, o, dp)
    inner = dp[1:, 1:]
    H = inner.min(axis=2, keepdims=True)
    inner[..., 1:] = H + np.minimum(inner[..., 1:] - H, saturate_at)
    mt = np.array(random.Random(seed).getstate()[1], dtype=np.uint32)
    cap = m + n + 2
    oa, om, ob = (C.create_string_buffer(cap) for _ in range(3))
    ln, nd = C.c_int64(0), C.c_int64(0)
    st = core.lib().gao_traceback_full(dp.reshape(-1), m, n, o, a, b, s1.encode(), s2.encode(), tab.sub, tab.K, tab.gh,
                                       mt, oa, om, ob, C.byref(ln), C.byref(nd))
    L = ln.value
    return st, (oa.raw[:L].decode(), om.raw[:L].decode(), ob.raw[:L].decode())


def test_gap_open_field_saturation_can_fail():
    """A traceback word's fields hold min(X - H, o + 1) and min(Y - H, o + 1); at o = 32766 that fills their 15 bits.
    Cells rebuilt from fields saturated at o + 1 walk as the real cells do, in every walk case at o = 32766.  From
    fields saturated at o, a difference above o looks like a tie with a gap opened from H; a walk meets one where the
    table's entries are of o's own magnitude, so the P16 and V16 cases must give other strings, at three seeds each
    (under the small tables a walk at o = 32766 hardly ever stands in a gap at such a cell: not asked of them)."""
    cases = [c for c in lc.all_single_cases() if c[4] == lc.O_MAX and lc.eligible(c) and c[2] * c[3] <= 2_000_000
             and c in set(lc.ROW_WALK) | {r[0] for r in lc.RC}]
    met, exact_cases = collections.Counter(), 0
    for case in cases:
        problem = lc.problem(case)
        cmat, s1, s2, o = problem
        differ = 0
        for seed in (1, 2, 3):
            r = core.align(s1, s2, cmat, o, np.array(random.Random(seed).getstate()[1], dtype=np.uint32), mode="full")
            exact = _walk_with_fields(problem, seed, o + 1)
            assert exact == (0 if r["status"] == "ok" else 1, tuple(r["strings"])), case
            differ += _walk_with_fields(problem, seed, o) != exact
        exact_cases += 1
        if case[0] in ("P16", "V16"):
            assert differ == 3, (case, differ)
            met[case[0]] += 1
    print("walk cases at o = 32766 that a field saturated at o changes at every seed:", dict(met), "of", exact_cases)
    assert dict(met) == {"V16": 1, "P16": 2} and exact_cases == 14
    # the batches with strings (batch_align, batch_sample) run at o = 32766: the same of every pair of the families
    # with entries of o's magnitude whose sides have at least 63 letters (a walk over a side of two or three letters
    # makes too few moves to stand at such a cell)
    batch = collections.Counter()
    problems = [(c[0], lc.problem(c)) for fam in (lc.P16, lc.P16A) for c in lc.batch_cases(fam, lc.BATCH_ALIGN_SHAPES, lc.O_MAX)]
    for fam, shapes in ((lc.V16, lc.V_BATCH_SHAPES), (lc.V32, lc.V32_SHAPES)):
        cmat, cases, _ = lc.v_batch_cases(fam, shapes, lc.O_MAX)
        problems += [(c[0], (cmat,) + lc.sequences(c) + (lc.O_MAX,)) for c in cases]
    for name, problem in problems:
        if min(len(problem[1]), len(problem[2])) < 63:
            continue
        for seed in (1, 2, 3):
            assert _walk_with_fields(problem, seed, lc.O_MAX) != _walk_with_fields(problem, seed, lc.O_MAX + 1), (name, seed)
        batch[name] += 1
    print("batch pairs at o = 32766 that a field saturated at o changes at every seed:", dict(batch))
    assert dict(batch) == EXPECTED_SATURATION_BATCH


EXPECTED_SATURATION_BATCH = {"P16": 17, "P16+a": 17, "V16": 11, "V32": 3}


def test_oracle_limit_costs_golden():
    """The reference at these magnitudes (Python's unbounded ints) against the oracle's int64: every record's status,
    cost, strings and final random state."""
    recs = json.load(open(os.path.join(GOLDEN, "limit_costs.json")))
    fams = {r["family"] for r in recs}
    assert fams >= {"P8", "P8+a", "P8+b", "P16", "K33", "K64", "V16", "Vphi", "V-"} and len(recs) >= 36
    assert sum(min(len(r["seq_1"]), len(r["seq_2"])) == 1 and r["gap_open_cost"] == lc.O_MAX for r in recs) >= 3
    for rec in recs:
        case = (rec["family"], rec["variant"], len(rec["seq_1"]), len(rec["seq_2"]), rec["gap_open_cost"])
        cmat = rec["costing_mat"]
        assert cmat == lc.table(case) and list(cmat.keys()) == list(lc.table(case).keys()), case
        if lc.is_v(case):
            assert rec["factor"] == lc.v_factor(*[case[0]] + list(case[2:]))
        random.seed(rec["seed"])
        res = core.align(rec["seq_1"], rec["seq_2"], cmat, rec["gap_open_cost"], core.mt_state_array())
        assert res["status"] == rec["status"], case
        assert res["cost"] == rec["cost"], case
        if rec["status"] == "ok":
            assert list(res["strings"]) == rec["strings"], case
        assert state_digest(core.mt_state_tuple(res["mt_out"])) == rec["state_after"], case
