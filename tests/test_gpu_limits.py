"""GPU parity at the limits the host checks admit.

The host proves that a problem is safe for the int32 kernels and picks their data widths (ga_check.h, load_problem,
the batch planner); the other GPU tests stay far inside every one of those limits -- table entries up to about 200,
stored values around 2^20, alphabets of at most 25 keys, gap opens up to 300.  Here the families of
tests/limit_costs.py go through every fill and walk path bit-exact against oracle.core under the same table: sub' at
+-127 and +-32767 and one past each, alphabets of 32 / 33 (the lane kernels' [K][32] tables and their decline), 64 /
65, 90 / 91, 128 / 129 (the batch table's LDS budget at 4, 2 and 1 bytes an entry) and 255 keys, tables and
caller-supplied boundaries scaled to the largest factor the guard admits (stored values of 2^25 to 2^29, beside the
sentinels HAND_SENT, BATCH_INF and the scan's 0x7fffffff), and gap open 32766, which fills a four-byte traceback
word's 15-bit fields exactly.  Every case asserts the path it took.  tests/test_limit_costs_cpu.py shows on the CPU
that the cases can fail and that they reach those magnitudes."""
import functools
import random

import numpy as np
import pytest

from tests import general_costs as gc
from tests import gpu_parity as gp
from tests import limit_costs as lc
from tests.conftest import set_knob

pytestmark = pytest.mark.gpu

RANGE_MSG = "problem exceeds the int32 score range of the device path"
PROFILE_MSG = "substitution costs exceed the int16 query profile"
WORD_MSG = "gap_open cost too large for the traceback word"


# ---------------------------------------------------------------- shared, cached references
@functools.lru_cache(maxsize=None)
def _problem(case):
    return lc.problem(case)


@functools.lru_cache(maxsize=None)
def _ref_chain(case, seed, count=1):
    return gp.ref_chain(_problem(case), seed, count)


@functools.lru_cache(maxsize=None)
def _oracle_cost(case):
    return gp.oracle_cost(_problem(case))


@functools.lru_cache(maxsize=None)
def _boundary(case):
    row0, col0 = lc.vb_boundary(case)
    return np.array(row0, dtype=np.int64), np.array(col0, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _full_reference(case):
    return gp.full_reference(_problem(case), _boundary(case) if case[0][:2] == "VB" else None)


def _int8_small_alphabet(case):
    """What the lane-skewed fill and the recompute walk take: an int8 profile and at most 32 keys."""
    return lc.profile_bytes(_problem(case)[0]) == 1 and lc.family_K(case[0]) <= 32


def _align(monkeypatch, case, seed, knobs, fill=None, walk=None):
    return gp.align(monkeypatch, _problem(case), seed, knobs, _ref_chain(case, seed)[0], fill=fill, walk=walk)


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


def _engine_error(excinfo, message):
    from globalign_amd import _native
    assert excinfo.type is _native.EngineError, excinfo.value
    assert "engine error -3:" in str(excinfo.value) and message in str(excinfo.value), excinfo.value


# ---------------------------------------------------------------- every cell, row scan
_FULL = list(lc.FULL_CELLS) + list(lc.FULL_CELLS_CUSTOM)


@pytest.mark.parametrize("t", [None, 2, 8])
@pytest.mark.parametrize("case", _FULL, ids=_ids(_FULL))
def test_every_cell_row_scan(monkeypatch, case, t):
    """Engine.fill(full=True): all three values of every interior cell against core.fill_full, un-shifted by the
    cell's own GV(i) + GH(j): sub' at +-127 and +-32767, 64 keys, the scaled table at 2^25 and caller-supplied
    boundary triples within 400 of +-(the guard's bound)."""
    custom = case[0][:2] == "VB"
    gp.full_cells(monkeypatch, _problem(case), t, _full_reference(case), custom=custom)


# ---------------------------------------------------------------- row scan + walk
@pytest.mark.parametrize("case", lc.ROW_WALK, ids=_ids(lc.ROW_WALK))
def test_row_scan_walk(monkeypatch, case):
    """The default single call (row scan with traceback words, stored-words walk) at one-, two- and four-byte words,
    o = 32766 filling the four-byte word's fields; 1150 rows wrap the profile rings of 1024, 512 and 256 rows that
    load_problem picks for 33 / 64 keys, 90 keys at int8 and 90 keys at int16."""
    _align(monkeypatch, case, seed=case[2] ^ case[3], knobs={}, fill="row", walk="stored")


def _load_only(K, scale):
    from globalign_amd import _native
    case = lc.K_(K, scale) + (3, 5, 6)
    cmat, s1, s2, o = _problem(case)
    tabs = _native.CostTables(cmat, o)
    eng = _native.Engine(0)
    try:
        eng.load(tabs.codes(s1), tabs.codes(s2), tabs)
    finally:
        eng.close()


@pytest.mark.parametrize("scale", [1, 5], ids=["int8", "int16"])
def test_largest_alphabet(monkeypatch, scale):
    """The largest alphabet Engine.load accepts, searched downwards from 255 by load alone, then filled: its profile
    ring has 256 rows at int8 and 128 at int16, and 1150 rows wrap it.  check_problem admits at most 255 keys, and
    at 255 the ring of 128 int16 rows still fits the workgroup's LDS beside the traceback stage, so the refusal
    "alphabet too large for the LDS query profile" has no input that reaches it; were a smaller K refused, K + 1 must
    be refused with that message."""
    largest = None
    for K in range(255, 200, -1):
        try:
            _load_only(K, scale)
            largest = K
            break
        except Exception as exc:
            assert "engine error -3:" in str(exc) and "alphabet too large for the LDS query profile" in str(exc), exc
    assert largest == 255
    for o in lc.WALK_OPENS:
        case = lc.K_(largest, scale) + lc.ROW_RING_SHAPE + (o,)
        s1, s2 = _problem(case)[1:3]
        assert lc.all_codes_occur(s1, largest) and lc.all_codes_occur(s2, largest)
        got, kind = gp.score(monkeypatch, _problem(case), {"GA_FILL_MODE": "row"}, ("row",))
        assert got == _oracle_cost(case)
    # the anti-diagonal kernel's profile ring has no room for its window at 255 keys (plan_fill: 128 rows are what
    # 64 KB hold, fewer than a workgroup's rows in flight): GA_FILL_MODE=diag runs the row scan too
    got, kind = gp.score(monkeypatch, _problem(case), {"GA_FILL_MODE": "diag"}, ("row",))
    assert got == _oracle_cost(case)


# ---------------------------------------------------------------- lane fill
_LANE_SCORE = [(td, nwc, c) for td in lc.LANE_TDS for nwc in (4, 8) for c in lc.lane_score_cases(td)]


@pytest.mark.parametrize("td,nwc,case", _LANE_SCORE, ids=[f"td{t}-nwc{w}-" + _ids([c])[0] for t, w, c in _LANE_SCORE])
def test_lane_score(monkeypatch, td, nwc, case):
    """GA_FILL_MODE=lane at every stripe width and both workgroup sizes; at TD 2 ten stripes, so that near-guard
    values cross the HBM hand-off rows polled against HAND_SENT."""
    knobs = {"GA_FILL_MODE": "lane", "GA_LANE_COLS_PER_LANE": td, "GA_FILL_NWC": nwc}
    assert _int8_small_alphabet(case)
    got, kind = gp.score(monkeypatch, _problem(case), knobs, ("lane", td))
    assert kind[3] == nwc, kind
    assert got == _oracle_cost(case)


@pytest.mark.parametrize("td", lc.LANE_TDS)
@pytest.mark.parametrize("case", lc.LANE_DECLINED, ids=_ids(lc.LANE_DECLINED))
def test_lane_declines(monkeypatch, td, case):
    """sub' = +128 (an int16 profile) and 33 keys (one more than the [K][32] sub' table holds): the row scan."""
    knobs = {"GA_FILL_MODE": "lane", "GA_LANE_COLS_PER_LANE": td, "GA_FILL_NWC": 4}
    assert not _int8_small_alphabet(case)
    got, kind = gp.score(monkeypatch, _problem(case), knobs, ("row",))
    assert got == _oracle_cost(case)


@pytest.mark.parametrize("case", lc.LANE_CUSTOM, ids=_ids(lc.LANE_CUSTOM))
def test_lane_mode_custom_boundary(monkeypatch, case):
    """Caller-supplied boundary triples at +-(the guard's bound) through the lane kernel (the planner's lane branch
    does not look at where the boundary came from); VB- over ten stripes, three workgroups, so that values near
    -2^29 cross the HBM hand-off rows polled against HAND_SENT."""
    row0, col0 = _boundary(case)
    knobs = {"GA_FILL_MODE": "lane", "GA_LANE_COLS_PER_LANE": 2, "GA_FILL_NWC": 4}
    got, kind = gp.score(monkeypatch, _problem(case), knobs, ("lane", 2), load_kw=dict(row0=row0, col0=col0))
    assert kind[3] == 4, kind
    if case[3] == lc.lane_handover_shape(2)[1]:
        assert kind[4] >= 3, kind
    assert got == gp.oracle_cost(_problem(case), (row0, col0))


@pytest.mark.parametrize("env", [{"GA_LANE_ASM": 0}, {"GA_LANE_DIRECT": 1}, {"GA_LANE_LEAN0": 0}],
                         ids=["asm0", "direct1", "lean0-0"])
def test_lane_handover_variants(monkeypatch, env):
    """The compiler's steps, the direct workgroup hand-off and the masked ramp, over three workgroups at TD 2."""
    knobs = dict(env, GA_FILL_MODE="lane", GA_LANE_COLS_PER_LANE=2, GA_FILL_NWC=4)
    got, kind = gp.score(monkeypatch, _problem(lc.LANE_HANDOVER), knobs, ("lane", 2))
    assert kind[4] >= 3, kind
    assert got == _oracle_cost(lc.LANE_HANDOVER)


_LANE_WALK = [(td, c) for td in (1, 2, 4) for c in lc.lane_walk_cases(td)]


@pytest.mark.parametrize("td,case", _LANE_WALK, ids=[f"td{t}-" + _ids([c])[0] for t, c in _LANE_WALK])
def test_lane_words_walk(monkeypatch, td, case):
    knobs = {"GA_FILL_MODE": "lane", "GA_LANE_COLS_PER_LANE": td, "GA_FILL_NWC": 4}
    _align(monkeypatch, case, seed=td + case[2], knobs=knobs, fill=("lane", td), walk="stored")


# ---------------------------------------------------------------- anti-diagonal fill
@pytest.mark.parametrize("td", [1, 2, 4])
@pytest.mark.parametrize("case", lc.DIAG, ids=_ids(lc.DIAG))
def test_diag_score(monkeypatch, td, case):
    knobs = {"GA_FILL_MODE": "diag", "GA_DIAG_COLS_PER_LANE": td}
    # (an int16 profile runs the anti-diagonal kernel at no more than 2 columns per lane)
    want_td = td if lc.profile_bytes(_problem(case)[0]) == 1 else min(td, 2)
    got, kind = gp.score(monkeypatch, _problem(case), knobs, ("diag", want_td))
    assert got == _oracle_cost(case)


# ---------------------------------------------------------------- recompute walk
@pytest.mark.parametrize("case,td,every", lc.RC, ids=[_ids([c])[0] + f"-td{t}-every{e}" for c, t, e in lc.RC])
def test_recompute_walk(monkeypatch, case, td, every):
    """GA_RC=1: the checkpointing lane fill and the walk that recomputes 64-row blocks, whose sub' table is the int8
    profile's bytes: -127 on every match, 32 keys, GV / GH / big at the guard's bound with either sign."""
    knobs = {"GA_RC": 1}
    if td is not None:
        knobs["GA_LANE_COLS_PER_LANE"] = td
    if every is not None:
        knobs["GA_RC_EVERY"] = every
    assert _int8_small_alphabet(case)
    kind = _align(monkeypatch, case, seed=case[2] + case[4], knobs=knobs, fill="rc", walk="rc")
    assert td is None or kind[1] == td, kind


@pytest.mark.parametrize("case", lc.RC_DECLINED, ids=_ids(lc.RC_DECLINED))
def test_recompute_walk_declines(monkeypatch, case):
    assert not _int8_small_alphabet(case)
    _align(monkeypatch, case, seed=case[2] + case[4], knobs={"GA_RC": 1}, fill="row", walk="stored")


# ---------------------------------------------------------------- banded traceback
@pytest.mark.parametrize("case,band_rows", lc.BANDED, ids=[_ids([c])[0] + f"-bh{b}" for c, b in lc.BANDED])
def test_banded_traceback(monkeypatch, case, band_rows):
    _align(monkeypatch, case, seed=case[3] ^ band_rows, knobs={"GA_TB_BAND_ROWS": band_rows}, walk="stored")


# ---------------------------------------------------------------- pipeline, slabs
@pytest.mark.parametrize("mode", ["lane", "row"])
@pytest.mark.parametrize("case", lc.PIPELINE, ids=_ids(lc.PIPELINE))
def test_pipeline_align_many(monkeypatch, case, mode):
    from globalign_amd import _native
    set_knob(monkeypatch, "GA_PIPE_MODE", mode)
    tabs, s1, s2 = gp.tables(_problem(case))
    ref = _ref_chain(case, 9, 3)
    eng = _native.Engine(0)
    try:
        eng.load(tabs.codes(s1), tabs.codes(s2), tabs)
        runs, mt_after = eng.align_many(gp.mt(9), s1, s2, 3)
    finally:
        eng.close()
    assert len(runs) == 3
    for (cost, strings, status), (cost_ref, strings_ref, status_ref, _) in zip(runs, ref):
        assert status == 0 and status_ref == "ok"
        assert cost == cost_ref and tuple(strings) == strings_ref
    assert tuple(np.asarray(mt_after, dtype=np.uint32).tolist()) == ref[-1][3]


@pytest.mark.parametrize("rc", [False, True], ids=["words", "rc"])
def test_slabs_in_process(monkeypatch, rc):
    from globalign_amd import distributed
    if rc:
        set_knob(monkeypatch, "GA_RC", 1)
    case = lc.SLABS
    tabs, s1, s2 = gp.tables(_problem(case))
    cost_ref, strings_ref, status_ref, mt_ref = _ref_chain(case, 21)[0]
    engines = [distributed.GpuSlabEngine(0) for _ in range(3)]
    try:
        cost, strings, status, mt_after = distributed.align_devices([0, 0, 0], s1, s2, tabs.codes(s1), tabs.codes(s2),
                                                                    tabs, gp.mt(21), engines=engines)
    finally:
        for e in engines:
            e.eng.close()
    assert status == 0 and status_ref == "ok"
    assert int(cost) == cost_ref and tuple(strings) == strings_ref
    assert tuple(np.asarray(mt_after, dtype=np.uint32).tolist()) == mt_ref


# ---------------------------------------------------------------- batches
def _batch_problems(kind):
    """The pairs of a batch as problems under one table -> (problems, gap open cost)."""
    if kind in ("V16", "Vphi", "V-", "V32"):
        fam = {"V16": lc.V16, "Vphi": lc.VPHI, "V-": lc.VNEG, "V32": lc.V32}[kind]
        shapes = lc.V32_SHAPES if kind == "V32" else lc.V_BATCH_SHAPES
        cmat, cases, _ = lc.v_batch_cases(fam, shapes, lc.O_MAX)
        return [(cmat,) + lc.sequences(c) + (lc.O_MAX,) for c in cases]
    fam, shapes = _BATCH_FAMILIES[kind]
    return [_problem(c) for c in lc.batch_cases(fam, shapes, lc.O_MAX)]


_BATCH_FAMILIES = {
    "P8": (lc.P8, lc.BATCH_COST_SHAPES), "P8+a": (lc.P8A, lc.BATCH_COST_SHAPES), "P8+b": (lc.P8B, lc.BATCH_COST_SHAPES),
    "P16": (lc.P16, lc.BATCH_COST_SHAPES), "P16+a": (lc.P16A, lc.BATCH_COST_SHAPES),
    "P16+b": (lc.P16B, lc.BATCH_COST_SHAPES),
    "K64x4": (lc.K_(64, 600), lc.K_BATCH_SHAPES), "K65x4": (lc.K_(65, 600), lc.K_BATCH_SHAPES),
    "K90x2": (lc.K_(90, 5), lc.K_BATCH_SHAPES), "K91x2": (lc.K_(91, 5), lc.K_BATCH_SHAPES),
    "K128x1": (lc.K_(128), lc.K_BATCH_SHAPES), "K129x1": (lc.K_(129), lc.K_BATCH_SHAPES),
}
# families whose sub' table leaves the kernel's 16 KB of LDS (65^2 x 4, 91^2 x 2, 129^2 x 1 bytes): every pair takes
# the single-pair fill, which refuses entries past int16 as the single call does
_ROUTED_OUT = {"K65x4": PROFILE_MSG, "K91x2": None, "K129x1": None}


@pytest.mark.parametrize("kind", list(_BATCH_FAMILIES) + ["V16", "Vphi", "V-", "V32"])
def test_batch_costs(kind):
    """Engine.batch_costs over the corner shapes (partial stripes: masked columns hold BATCH_INF beside real values)
    at o = 32766: every profile width of the kernel's table, 4-byte entries included, and both sides of the table's
    LDS budget.  A table that does not fit sends every pair to the single-pair fill; the call then reports what the
    single call reports (K65 at 4 bytes: the int16 profile's refusal)."""
    from globalign_amd import _native
    problems = _batch_problems(kind)
    assert len(problems) >= 5
    K, qb = len(problems[0][0]), lc.profile_bytes(problems[0][0]) or 4
    assert (K * K * qb > 16 * 1024) == (kind in _ROUTED_OUT), (K, qb)
    if kind == "K64x4":
        assert K * K * qb == 16 * 1024
    tabs, codes, _, seq_off, pa, pb = gp.batch_inputs(problems)
    eng = _native.Engine(0)
    try:
        if _ROUTED_OUT.get(kind):
            with pytest.raises(Exception) as excinfo:
                eng.batch_costs(codes, seq_off, pa, pb, tabs)
            _engine_error(excinfo, _ROUTED_OUT[kind])
            return
        costs = eng.batch_costs(codes, seq_off, pa, pb, tabs)
    finally:
        eng.close()
    want = [gp.oracle_cost(p) for p in problems]
    bad = [(len(p[1]), len(p[2]), int(g), w) for p, g, w in zip(problems, costs, want) if int(g) != w]
    assert not bad, bad[:6]


_ALIGN_KINDS = ["P8", "P8+a", "P16", "P16+a", "V16", "Vphi", "V32"]
_BATCH_SEEDS = [0, 5, 5, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1, 2 ** 40]


@functools.lru_cache(maxsize=None)
def _align_batch(kind):
    """(problems, seeds, the oracle's result per pair) of a batch with strings: BATCH_ALIGN_SHAPES cut to the guard."""
    if kind in ("V16", "Vphi", "V32"):
        problems = _batch_problems(kind)
    else:
        problems = [_problem(c) for c in lc.batch_cases(_BATCH_FAMILIES[kind][0], lc.BATCH_ALIGN_SHAPES, lc.O_MAX)]
    seeds = [(_BATCH_SEEDS[k % 8] + (k // 8) * 1000) % 2 ** 64 for k in range(len(problems))]
    from oracle import core
    want = [core.align(p[1], p[2], p[0], p[3], gp.mt(s)) for p, s in zip(problems, seeds)]
    return problems, seeds, want


def _check_strings(problems, want, costs, status, lengths, offsets, bufs, slot_of):
    from globalign_amd import _native
    bad = []
    for k, (p, r) in enumerate(zip(problems, want)):
        f = slot_of(k)
        lo, hi = int(offsets[f]), int(offsets[f]) + int(lengths[f])
        got = tuple(buf[lo:hi].tobytes().decode() for buf in bufs)
        ok = int(costs[k]) == r["cost"] and int(status[f]) == (0 if r["status"] == "ok" else _native.GA_TB_INDEX_ERROR)
        if ok and r["status"] == "ok":
            ok = got == tuple(r["strings"])
        if not ok:
            bad.append((len(p[1]), len(p[2]), int(costs[k]), r["cost"], int(status[f]), r["status"]))
    assert not bad, bad[:6]


@pytest.mark.parametrize("tables", ["host", "device"])
@pytest.mark.parametrize("kind", _ALIGN_KINDS)
def test_batch_align(kind, tables):
    """Engine.batch_align at o = 32766, where o + 1 fills a four-byte word's 15-bit fields.  The walks that stand at
    differences above o are those of P16, P16+a, V16 and V32, whose entries are of o's magnitude
    (tests/test_limit_costs_cpu.py::test_gap_open_field_saturation_can_fail); under P8, P8+a and Vphi the fields
    are as wide but a walk hardly ever meets a saturated one."""
    from globalign_amd import _native
    problems, seeds, want = _align_batch(kind)
    tabs, codes, chars, seq_off, pa, pb = gp.batch_inputs(problems)
    eng = _native.Engine(0)
    try:
        costs, status, lengths, offsets, bufs = eng.batch_align(codes, seq_off, pa, pb, tabs, seeds, chars,
                                                                rng_tables=tables)
        info = eng.batch_align_info()
    finally:
        eng.close()
    in_kernel = sum(min(len(p[1]), len(p[2])) >= 2 for p in problems)
    assert info["device_items"] + info["host_items"] == in_kernel, info
    _check_strings(problems, want, costs, status, lengths, offsets, bufs, lambda k: k)


@pytest.mark.parametrize("kind", ["P8", "P16+a", "Vphi", "V32"])
def test_batch_sample(kind):
    """Engine.batch_sample, three samples a pair; sample 0 of each pair has the batch_align seed."""
    from globalign_amd import _native
    from oracle import core
    problems, seeds, want = _align_batch(kind)
    P = len(problems)
    tabs, codes, chars, seq_off, pa, pb = gp.batch_inputs(problems)
    sample_off = np.arange(0, 3 * P + 1, 3, dtype=np.int64)
    all_seeds = [s for k in range(P) for s in (seeds[k], 7000 + k, 2 ** 33 + k)]
    eng = _native.Engine(0)
    try:
        costs, status, lengths, offsets, bufs = eng.batch_sample(codes, seq_off, pa, pb, tabs, sample_off, all_seeds,
                                                                 chars)
        info = eng.batch_sample_info()
    finally:
        eng.close()
    in_kernel = sum(min(len(p[1]), len(p[2])) >= 2 for p in problems)
    assert info["filled_pairs"] == in_kernel and info["walk_items"] == 3 * in_kernel, info
    for t in range(3):
        if t:
            want = [core.align(p[1], p[2], p[0], p[3], gp.mt(all_seeds[3 * k + t])) for k, p in enumerate(problems)]
        _check_strings(problems, want, costs, status, lengths, offsets, bufs, lambda k: 3 * k + t)


@pytest.mark.parametrize("kind,in_kernel", [("K64x4", True), ("K65x4", False), ("K90x2", True), ("K91x2", False),
                                            ("K128x1", True), ("K129x1", False)])
def test_batch_table_routing_edges(kind, in_kernel):
    """The batch table's LDS budget, by the counts the engine reports (batch_costs reports none; the align and sample
    planners route through the same plan_batch_routed): 64^2 x 4, 90^2 x 2 and 128^2 x 1 bytes stay in the kernels,
    one key more sends every pair to the single-pair path -- which refuses the entries past int16 of K65."""
    from globalign_amd import _native
    from oracle import core
    problems = [p for p in _batch_problems(kind) if (len(p[1]), len(p[2])) in ((65, 129), (257, 64))]
    assert len(problems) == 2
    tabs, codes, chars, seq_off, pa, pb = gp.batch_inputs(problems)
    sample_off = np.array([0, 2, 4], dtype=np.int64)
    seeds = [11, 2 ** 33, 12, 13]
    eng = _native.Engine(0)
    try:
        if kind == "K65x4":
            for call in (lambda: eng.batch_align(codes, seq_off, pa, pb, tabs, seeds[:2], chars),
                         lambda: eng.batch_sample(codes, seq_off, pa, pb, tabs, sample_off, seeds, chars)):
                with pytest.raises(Exception) as excinfo:
                    call()
                _engine_error(excinfo, PROFILE_MSG)
            return
        acosts = eng.batch_align(codes, seq_off, pa, pb, tabs, seeds[:2], chars)[0]
        ainfo = eng.batch_align_info()
        costs, status, lengths, offsets, bufs = eng.batch_sample(codes, seq_off, pa, pb, tabs, sample_off, seeds, chars)
        info = eng.batch_sample_info()
    finally:
        eng.close()
    assert ainfo["device_items"] + ainfo["host_items"] == (2 if in_kernel else 0), ainfo
    if in_kernel:
        assert (info["filled_pairs"], info["single_fill_pairs"], info["looped_pairs"]) == (2, 0, 0), info
        assert info["walk_items"] == 4, info
    else:
        assert info["filled_pairs"] == 0 and info["single_fill_pairs"] + info["looped_pairs"] == 2, info
        # (a pair the single-pair fill filled once is still walked sample by sample by batch_walks_kernel)
        assert info["walk_items"] == 2 * info["single_fill_pairs"], info
    want = [gp.oracle_cost(p) for p in problems]
    assert [int(c) for c in costs] == want and [int(c) for c in acosts] == want
    if "".join(problems[0][1:3]).isascii():  # (K128 / K129 have codes without characters: costs and counts only)
        for f, seed in enumerate(seeds):
            p = problems[f // 2]
            r = core.align(p[1], p[2], p[0], p[3], gp.mt(seed))
            lo, hi = int(offsets[f]), int(offsets[f]) + int(lengths[f])
            assert r["status"] == "ok" and int(status[f]) == 0
            assert tuple(buf[lo:hi].tobytes().decode() for buf in bufs) == tuple(r["strings"]), (kind, f)


@pytest.mark.parametrize("kind", ["Vphi", "P16"])
def test_batch_align_large_route(monkeypatch, kind):
    """GA_BATCH_ALIGN_MAX_CELLS=4096: two pairs above it take the single-pair path out of the batch."""
    from globalign_amd import _native
    set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", 4096)
    problems, seeds, want = _align_batch(kind)
    pick = [k for k, p in enumerate(problems) if (len(p[1]), len(p[2])) in ((65, 129), (300, 300), (64, 64), (3, 65))]
    assert len(pick) == 4
    problems, seeds, want = [problems[k] for k in pick], [seeds[k] for k in pick], [want[k] for k in pick]
    tabs, codes, chars, seq_off, pa, pb = gp.batch_inputs(problems)
    eng = _native.Engine(0)
    try:
        costs, status, lengths, offsets, bufs = eng.batch_align(codes, seq_off, pa, pb, tabs, seeds, chars)
        info = eng.batch_align_info()
    finally:
        eng.close()
    assert info["device_items"] + info["host_items"] == 2, info  # 64 x 64 and 3 x 65 stay in the kernel
    _check_strings(problems, want, costs, status, lengths, offsets, bufs, lambda k: k)


# ---------------------------------------------------------------- refusals
def _load(problem):
    from globalign_amd import _native
    tabs, s1, s2 = gp.tables(problem)
    eng = _native.Engine(0)
    try:
        eng.load(tabs.codes(s1), tabs.codes(s2), tabs)
    finally:
        eng.close()


@pytest.mark.parametrize("fam", [lc.P16A, lc.P16B], ids=["+32768", "-32768"])
def test_single_call_refuses_past_int16(fam):
    with pytest.raises(Exception) as excinfo:
        _load(_problem(fam + (65, 130, 6)))
    _engine_error(excinfo, PROFILE_MSG)


@pytest.mark.parametrize("family,m,n,o,message", [("V16", 1100, 600, lc.O_MAX, PROFILE_MSG), ("V16", 4096, 1024, 5, RANGE_MSG),
                                                  ("Vphi", 777, 2049, 7, RANGE_MSG), ("V-", 2049, 700, 5, RANGE_MSG)])
def test_load_refuses_factor_plus_one(family, m, n, o, message):
    """The first factor the restated guard refuses is the first one the engine refuses; the factor itself loads."""
    s1, s2 = lc.sequences((family, 0, m, n, o))
    _load((lc.v_table(family, m, n, o), s1, s2, o))
    with pytest.raises(Exception) as excinfo:
        _load((lc.v_table(family, m, n, o, excess=1), s1, s2, o))
    _engine_error(excinfo, message)


def _batch_calls(eng, problems, tabs=None):
    """The three batched calls over `problems` as thunks."""
    tabs0, codes, chars, seq_off, pa, pb = gp.batch_inputs(problems)
    tabs = tabs or tabs0
    P = len(problems)
    return {"costs": lambda: eng.batch_costs(codes, seq_off, pa, pb, tabs),
            "align": lambda: eng.batch_align(codes, seq_off, pa, pb, tabs, list(range(P)), chars),
            "sample": lambda: eng.batch_sample(codes, seq_off, pa, pb, tabs, np.arange(P + 1, dtype=np.int64),
                                               list(range(P)), chars)}


def test_gap_open_32767_refused():
    """o = 32767: o + 1 no longer fits a 15-bit field.  The single, batch-score, batch-align and sample calls."""
    from globalign_amd import _native
    cmat, s1, s2, _ = _problem(lc.P8 + (65, 130, 6))
    with pytest.raises(Exception) as excinfo:
        _load((cmat, s1, s2, 32767))
    _engine_error(excinfo, WORD_MSG)
    _load((cmat, s1, s2, 32766))
    eng = _native.Engine(0)
    try:
        for name, call in _batch_calls(eng, [(cmat, s1, s2, 32767), (cmat, s2, s1, 32767)]).items():
            with pytest.raises(Exception) as excinfo:
                call()
            _engine_error(excinfo, "pair 0: " + WORD_MSG)
    finally:
        eng.close()


@pytest.mark.parametrize("family", ["Vphi", "V-", "V32"])
def test_batch_refuses_factor_plus_one_of_one_pair(family):
    """A batch under the table one factor past what its largest pair admits: "pair 1: ..." while the pairs around it
    are fine; under the factor itself the batch runs."""
    from globalign_amd import _native
    shapes = [(64, 64), (65, 70), (3, 65)] if family == "V32" else [(64, 64), (300, 300), (65, 129)]
    o = lc.O_MAX
    f = lc.v_factor(family, *shapes[1], o)
    assert all(lc.v_factor(family, m, n, o) > f for m, n in (shapes[0], shapes[2]))
    seqs = [lc.sequences((family, 0, m, n, o)) for m, n in shapes]
    eng = _native.Engine(0)
    try:
        good = [(lc._v_table(family, f),) + s + (o,) for s in seqs]
        costs = _batch_calls(eng, good)["costs"]()
        assert [int(c) for c in costs] == [gp.oracle_cost(p) for p in good]
        bad = [(lc._v_table(family, f + 1),) + s + (o,) for s in seqs]
        for name, call in _batch_calls(eng, bad).items():
            with pytest.raises(Exception) as excinfo:
                call()
            _engine_error(excinfo, "pair 1: " + RANGE_MSG)
    finally:
        eng.close()


# ---------------------------------------------------------------- public API
def _api_rows():
    """general_costs' family-S score matrix times 1000: a costing matrix with an int16 profile."""
    letters, rows = gc.api_score_rows(gc.S1[1])
    return letters, [[1000 * v for v in row] for row in rows]


def test_public_api_int16_matrix_gap_open_32766(tmp_path):
    """find_global_alignment, score_pairs and align_pairs under a .mtx file whose costing matrix needs the int16
    profile, at gap_open_score = -32766."""
    import globalign_amd as ga
    from oracle import core, transform
    letters, rows = _api_rows()
    path = gc.write_mtx(tmp_path / "limit.mtx", letters, rows)
    smat = transform.read_mtx_rows(letters, rows)
    cmat = transform.scores_to_costs(smat, transform.max_val(smat))
    assert lc.profile_bytes(cmat) == 2
    kw = dict(scoring_mat_path=path, gap_open_score=-lc.O_MAX)
    shapes = [(130, 321), (65, 129), (64, 64), (3, 65), (300, 300)]
    pairs = [(gc.splitmix_seq(m, 9100 + m), gc.splitmix_seq(n, 9200 + n)) for m, n in shapes]
    assert all(lc.single_accepts(cmat, m, n, lc.O_MAX) for m, n in shapes)

    def score(cost, s1, s2):
        return transform.cost_to_score(cost, len(s1), len(s2), transform.max_val(smat))

    s1, s2 = pairs[0]
    ref = core.align(s1, s2, cmat, lc.O_MAX, gp.mt(3))
    random.seed(3)
    r = ga.find_global_alignment(seq_1=s1, seq_2=s2, **kw)
    assert r.gap_open_cost == lc.O_MAX and r.costing_mat == cmat
    assert r.cost == ref["cost"] and r.score == score(ref["cost"], s1, s2)
    assert (r.seq_1_aligned, r.middle_part, r.seq_2_aligned) == tuple(ref["strings"])
    assert random.getstate()[1] == tuple(int(x) for x in ref["mt_out"])
    want = np.array([gc.oracle_cost(cmat, a, b, lc.O_MAX) for a, b in pairs], dtype=np.int64)
    scores = np.array([score(int(c), a, b) for c, (a, b) in zip(want, pairs)], dtype=np.int64)
    al = ga.GlobalAligner(**kw)
    res = al.score_pairs([p[0] for p in pairs], [p[1] for p in pairs])
    assert np.array_equal(res.costs, want) and np.array_equal(res.scores, scores)
    aligned = al.align_pairs([p[0] for p in pairs], [p[1] for p in pairs], seeds=2 ** 32 - 2)
    assert np.array_equal(aligned.costs, want) and np.array_equal(aligned.scores, scores)
    for k, (a, b) in enumerate(pairs):
        rk = core.align(a, b, cmat, lc.O_MAX, gp.mt(2 ** 32 - 2 + k))
        assert rk["status"] == "ok"
        assert (aligned.seq_1_aligned[k], aligned.middle_part[k], aligned.seq_2_aligned[k]) == tuple(rk["strings"]), k
