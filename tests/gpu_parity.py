"""What the GPU parity tests under explicit cost tables share (tests/test_gpu_general_costs.py,
tests/test_gpu_limits.py, tests/test_gpu_tie_classes.py, tests/test_gpu_path_geometry.py): one engine call of a
problem against the oracle's result for it.  A problem is a tuple (costing dict, seq_1, seq_2, gap open cost); the
callers keep their own case lists and cached references."""
import random

import numpy as np

from tests.conftest import set_knob, del_knob


def mt(seed):
    """The 625 words of random.seed(seed)'s state."""
    return np.array(random.Random(seed).getstate()[1], dtype=np.uint32)


def ref_chain(problem, seed, count=1):
    """`count` consecutive oracle alignments of a problem from random.seed(seed): [(cost, strings, status, mt words)]."""
    from oracle import core
    cmat, s1, s2, o = problem
    state, out = mt(seed), []
    for _ in range(count):
        r = core.align(s1, s2, cmat, o, state)
        state = np.asarray(r["mt_out"], dtype=np.uint32).copy()
        out.append((r["cost"], tuple(r["strings"]), r["status"], tuple(state.tolist())))
    return out


def oracle_cost(problem, boundary=None):
    """min of the last cell of the oracle's score fill, over the reference's boundary or caller-supplied triples."""
    from oracle import core
    cmat, s1, s2, o = problem
    tab = core.Tables(cmat)
    a, b = tab.codes(s1), tab.codes(s2)
    if boundary is None:
        row0, col0 = core.boundary(tab, a, b, o, (tab.max_cost + 1) * max(len(a), len(b)))
    else:
        row0, col0 = (np.ascontiguousarray(x, dtype=np.int64) for x in boundary)
    return int(min(core.fill_score(tab, a, b, o, row0, col0)))


def tables(problem):
    """-> (CostTables, seq_1, seq_2) of a problem."""
    from globalign_amd import _native
    cmat, s1, s2, o = problem
    return _native.CostTables(cmat, o), s1, s2


def _align_on(eng, problem, seed, ref, fill, walk):
    """One Engine.align of a problem on an open engine against ref; -> fill_kind()."""
    from globalign_amd import _native
    tabs, s1, s2 = tables(problem)
    cost_ref, strings_ref, status_ref, mt_ref = ref
    eng.load(tabs.codes(s1), tabs.codes(s2), tabs)
    cost, strings, status, mt_after = eng.align(mt(seed), s1, s2)
    kind, wkind = eng.fill_kind(), eng.walk_kind()
    if fill is not None:
        want = fill if isinstance(fill, tuple) else (fill,)
        assert kind[:len(want)] == want, (kind, want)
    if walk is not None:
        assert wkind == walk, (wkind, kind)
    assert status == (0 if status_ref == "ok" else _native.GA_TB_INDEX_ERROR)
    assert int(cost) == cost_ref
    assert tuple(strings) == strings_ref
    assert tuple(np.asarray(mt_after, dtype=np.uint32).tolist()) == mt_ref
    return kind


def align(monkeypatch, problem, seed, knobs, ref, fill=None, walk=None):
    """Engine.align of a problem under `knobs` against ref = (cost, strings, status, mt words), the oracle's result
    from random.seed(seed): cost, strings, status and every MT word; fill / walk: what fill_kind() / walk_kind() must
    report (fill: a kind, or (kind, columns per lane))."""
    return align_cases(monkeypatch, [(problem, seed, ref)], knobs, fill, walk)[0]


def align_cases(monkeypatch, items, knobs, fill=None, walk=None):
    """align() of every (problem, seed, ref) of `items` on ONE engine created under `knobs` (a list of small cases
    spends its time creating engines otherwise) -> [fill_kind()]; a failure names the item's index."""
    from globalign_amd import _native
    for k, v in knobs.items():
        set_knob(monkeypatch, k, v)
    eng = _native.Engine(0)
    kinds = []
    try:
        for q, (problem, seed, ref) in enumerate(items):
            try:
                kinds.append(_align_on(eng, problem, seed, ref, fill, walk))
            except AssertionError as e:
                raise AssertionError(f"item {q} (o = {problem[3]}): {e}") from e
    finally:
        eng.close()
    return kinds


def score(monkeypatch, problem, knobs, fill, load_kw=None):
    """Engine.fill(traceback=False) under `knobs` -> (cost, fill_kind()); fill: the fill_kind() prefix that must have
    run."""
    from globalign_amd import _native
    for k, v in knobs.items():
        set_knob(monkeypatch, k, v)
    cmat, s1, s2, o = problem
    tabs = _native.CostTables(cmat, o)
    eng = _native.Engine(0)
    try:
        eng.load(tabs.codes(s1), tabs.codes(s2), tabs, **(load_kw or {}))
        cost = int(eng.fill(traceback=False)[0])
        kind = eng.fill_kind()
    finally:
        eng.close()
    assert kind[:len(fill)] == fill, (kind, fill)
    return cost, kind


def full_reference(problem, boundary=None):
    """core.fill_full over the reference's boundary, or over caller triples boundary = (row0, col0)
    -> (dp, row0, col0), dp read-only."""
    from oracle import core
    cmat, s1, s2, o = problem
    tab = core.Tables(cmat)
    a, b = tab.codes(s1), tab.codes(s2)
    m, n = len(a), len(b)
    if boundary is not None:
        row0, col0 = (np.ascontiguousarray(x, dtype=np.int64) for x in boundary)
    else:
        row0, col0 = core.boundary(tab, a, b, o, (tab.max_cost + 1) * max(m, n))
    dp = np.zeros((m + 1, n + 1, 3), np.int64)
    dp[0, :, :] = row0.reshape(n + 1, 3)
    dp[:, 0, :] = col0.reshape(m + 1, 3)
    core.fill_full(tab, a, b, o, dp)
    dp.setflags(write=False)
    return dp, row0, col0


def full_cells(monkeypatch, problem, t, reference, custom=False):
    """Engine.fill(full=True) at t columns per lane (None: the default) against reference = full_reference(...):
    the cost and all three values of every interior cell; custom: load the reference's row0 / col0."""
    from globalign_amd import _native
    if t is None:
        del_knob(monkeypatch, "GA_COLS_PER_LANE")
    else:
        set_knob(monkeypatch, "GA_COLS_PER_LANE", t)
    dp, row0, col0 = reference
    tabs, s1, s2 = tables(problem)
    eng = _native.Engine(0)
    try:
        eng.load(tabs.codes(s1), tabs.codes(s2), tabs, **(dict(row0=row0, col0=col0) if custom else {}))
        cost, full = eng.fill(full=True)
        kind = eng.fill_kind()
    finally:
        eng.close()
    assert kind[0] == "row", kind
    assert int(cost) == int(dp[-1, -1].min())
    bad = np.argwhere(full[1:, 1:].astype(np.int64) != dp[1:, 1:])
    assert bad.size == 0, [(int(i) + 1, int(j) + 1, int(k), int(full[i + 1, j + 1, k]), int(dp[i + 1, j + 1, k]))
                           for i, j, k in bad[:6]]


def batch_inputs(problems):
    """(CostTables, codes, chars, seq_off, pair_a, pair_b) of a batch whose pair k is problems[k] (all under the first
    problem's table and gap open cost)."""
    from globalign_amd import _native
    cmat, _, _, o = problems[0]
    tabs = _native.CostTables(cmat, o)
    seqs = [s for p in problems for s in p[1:3]]
    codes = np.frombuffer(b"".join(tabs.codes(s) for s in seqs), dtype=np.uint8)
    # one byte per letter: the text itself where it is ASCII (batches with strings), else the codes (scores only)
    text = "".join(seqs)
    chars = np.frombuffer(text.encode(), dtype=np.uint8) if text.isascii() else codes
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    P = len(problems)
    return tabs, codes, chars, seq_off, np.arange(0, 2 * P, 2), np.arange(1, 2 * P, 2)
