"""Every tie class on every traceback decoder and word width.

A walked cell's decision -- (entering level, argmin set, a_i == b_j) picks the tie-break entry's bit field -- has 42
set classes and, as the LUT decoders key it, 138 joint classes (tests/tie_classes.py).  The suite's i.i.d. sequences
under everyday costs enter about half of the set classes and a third of the joint ones, so a wrong LUT
entry, a `<=` for `<` in a field's flags, a dropped term of a rank set or a misplaced field of a device-made
tie-break entry could pass every other test.  Here the case lists of tests/tie_classes.py, which enter every tie class
at least 8 times, every single-minimum class twice and every joint class once per (path, width)
(tests/test_tie_classes_cpu.py proves that on the CPU oracle; the classes short of their count are named there), go
through each word encoder and each decoder at one-, two- and four-byte words, bit-exact against oracle.core: cost,
the three strings, status and all 625 MT words where the path returns them.  One test per (path, width) runs its
whole list on one engine.

The lane fill and the recompute walk take int8 query profiles only: their two- and four-byte lists are the
admissible ones (tie_classes.width_cases(width, int8=True))."""
import functools

import numpy as np
import pytest

from tests import gpu_parity as gp
from tests import tie_classes as tc
from tests.conftest import set_knob

pytestmark = pytest.mark.gpu

WIDTHS = tc.WIDTHS
SAMPLES = 3


@functools.lru_cache(maxsize=None)
def _problem(case, k):
    return tc.scaled_problem(case, k)


@functools.lru_cache(maxsize=None)
def _ref(case, k, seed, count=1):
    """`count` chained oracle alignments of a (scaled) case from random.seed(seed)."""
    return gp.ref_chain(_problem(case, k), seed, count)


def _items(width, int8=False):
    """[(problem, seed, oracle result)] of a width's list."""
    out = []
    for case, k in tc.width_cases(width, int8):
        assert tc.tb_word_bytes(case[2] * k) == width
        out.append((_problem(case, k), tc.case_seed(case), _ref(case, k, tc.case_seed(case))[0]))
    return out


# ---------------------------------------------------------------- single calls: every fill's encoder, both walks
@pytest.mark.parametrize("width", WIDTHS)
def test_row_scan_stored_walk(monkeypatch, width):
    """fill_kernel's words, load_tile_b1 / load_tile<2> / load_tile<4>."""
    gp.align_cases(monkeypatch, _items(width), {}, fill="row", walk="stored")


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("td", [1, 2])
def test_lane_words_stored_walk(monkeypatch, td, width):
    """The lane fill's rotated windows as the word encoder."""
    knobs = {"GA_FILL_MODE": "lane", "GA_LANE_COLS_PER_LANE": td, "GA_FILL_NWC": 4}
    kinds = gp.align_cases(monkeypatch, _items(width, int8=True), knobs, fill=("lane", td), walk="stored")
    assert all(kind[3] == 4 for kind in kinds), kinds


def _rc_columns(td, width, every=64):
    """The columns per lane the recompute fill keeps of `td` asked for (ga_plan.h plan_rc_fill, restated): a worker
    stages 64 * TD columns of (every + 136) words, 16-byte aligned, an a-window and an edge window, and must fit the
    128 KiB beside the walk's torus with 1 KiB to spare; the stripes halve until it does.  These problems take the
    densest checkpoint spacing, 64 steps."""
    while td > 1:
        sp = ((every + 136) * width + 16 + 15) & ~15
        if 1024 + 64 * td * sp + (every + 256) * 12 <= 256 * 256 * 2:
            break
        td //= 2
    return td


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("td", [2, 4])
def test_recompute_walk(monkeypatch, td, width):
    """ga_rcwalk.hip's workers as the encoder, the RC instantiations of the three decoders (the word walk: the
    tie-to-tie walk of experiments builds is switched off).  A worker's block of four-byte words at 4 columns per
    lane does not fit LDS beside the walk's torus: the stripes narrow to 2, which the engine reports."""
    knobs = {"GA_RC": 1, "GA_LANE_COLS_PER_LANE": td, "GA_RC_JUMP": 0}
    assert [_rc_columns(4, w) for w in WIDTHS] == [4, 4, 2] and _rc_columns(2, 4) == 2
    gp.align_cases(monkeypatch, _items(width, int8=True), knobs, fill=("rc", _rc_columns(td, width)), walk="rc")


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("band_rows", [16, 64])
def test_banded_refills(monkeypatch, band_rows, width):
    """The banded refills as the encoder; the walk handed on at each band top, level and all.  No fill kind is
    asserted: fill_kind() does not tell a banded traceback from a whole one; the bands are forced by
    m = 500 >= 2 * band_rows (as tests/test_gpu_general_costs.py::test_banded_traceback relies on)."""
    gp.align_cases(monkeypatch, _items(width), {"GA_TB_BAND_ROWS": band_rows}, walk="stored")


# ---------------------------------------------------------------- pipeline
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mode,chain", [("lane", None), ("row", None), ("lane", 1)], ids=["lane", "row", "lane-chain"])
def test_pipeline_align_many(monkeypatch, mode, chain, width):
    """Engine.align_many, three alignments chained through the random state, under both pipeline fill kernels and
    with the walks chained in one launch (GA_PIPE_CHAIN=1: walk_body's ring path).  The pipeline's lane fills take
    int8 profiles only (ga_pipe.h plan), at 4 columns per lane with one-byte words and 2 otherwise: the lane modes
    run the int8 lists, and fill_kind() after every call must name the kernel the mode asks for."""
    from globalign_amd import _native
    set_knob(monkeypatch, "GA_PIPE_MODE", mode)
    if chain is not None:
        set_knob(monkeypatch, "GA_PIPE_CHAIN", chain)
    want = ("lane", 4 if width == 1 else 2) if mode == "lane" else ("row",)
    eng = _native.Engine(0)
    try:
        for q, (case, k) in enumerate(tc.width_cases(width, int8=mode == "lane")):
            seed = tc.case_seed(case)
            problem, ref = _problem(case, k), _ref(case, k, seed, 3)
            tabs, s1, s2 = gp.tables(problem)
            eng.load(tabs.codes(s1), tabs.codes(s2), tabs)
            runs, mt_after = eng.align_many(gp.mt(seed), s1, s2, 3)
            kind = eng.fill_kind()
            assert kind[:len(want)] == want, (q, case, k, kind)
            assert len(runs) == 3
            for (cost, strings, status), (cost_ref, strings_ref, status_ref, _) in zip(runs, ref):
                assert status == 0 and status_ref == "ok", (q, case, k)
                assert cost == cost_ref and tuple(strings) == strings_ref, (q, case, k)
            assert tuple(np.asarray(mt_after, dtype=np.uint32).tolist()) == ref[-1][3], (q, case, k)
    finally:
        eng.close()


# ---------------------------------------------------------------- batches (one table and gap open cost per call)
def _groups(width):
    """The width's list by (table, gap open cost): {key: [(case, k)]}, in list order."""
    out = {}
    for case, k in tc.width_cases(width):
        out.setdefault((case[0], case[1], case[2], k), []).append((case, k))
    return out


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("route", ["host", "device"])
def test_batch_align(monkeypatch, route, width):
    """batch_align_kernel's words and the batch walker's decode, every case of the width in a batch with the cases
    of its table, one seed per pair; tie-break entries made by the host and by batch_rng_kernel."""
    from globalign_amd import _native
    set_knob(monkeypatch, "GA_BATCH_RNG_DEVICE_MAX_STEPS", 8192)
    eng = _native.Engine(0)
    try:
        for key, members in _groups(width).items():
            problems = [_problem(c, k) for c, k in members]
            seeds = [tc.case_seed(c) for c, _ in members]
            tabs, codes, chars, seq_off, pa, pb = gp.batch_inputs(problems)
            costs, status, lengths, offsets, bufs = eng.batch_align(codes, seq_off, pa, pb, tabs, seeds, chars,
                                                                    rng_tables=route)
            info = eng.batch_align_info()
            P = len(members)
            assert (info["device_items"], info["host_items"], info["fell_back"]) == \
                ((P, 0, False) if route == "device" else (0, P, False)), (key, info)
            for q, ((case, k), seed) in enumerate(zip(members, seeds)):
                cost_ref, strings_ref, status_ref, _ = _ref(case, k, seed)[0]
                lo, hi = int(offsets[q]), int(offsets[q]) + int(lengths[q])
                got = tuple(buf[lo:hi].tobytes().decode() for buf in bufs)
                assert int(status[q]) == 0 and status_ref == "ok", (case, k)
                assert int(costs[q]) == cost_ref and got == strings_ref, (case, k)
    finally:
        eng.close()


@pytest.mark.parametrize("width", WIDTHS)
def test_batch_sample(width):
    """batch_words_kernel + batch_walks_kernel: three seeded walks of every pair from one fill of it."""
    from globalign_amd import _native
    eng = _native.Engine(0)
    try:
        for key, members in _groups(width).items():
            problems = [_problem(c, k) for c, k in members]
            P = len(members)
            seeds = [tc.case_seed(c) + t for c, _ in members for t in range(SAMPLES)]
            tabs, codes, chars, seq_off, pa, pb = gp.batch_inputs(problems)
            sample_off = np.arange(P + 1, dtype=np.int64) * SAMPLES
            costs, status, lengths, offsets, bufs = eng.batch_sample(codes, seq_off, pa, pb, tabs, sample_off, seeds,
                                                                     chars)
            info = eng.batch_sample_info()
            assert (info["filled_pairs"], info["walk_items"], info["single_fill_pairs"], info["looped_pairs"]) == \
                (P, SAMPLES * P, 0, 0), (key, info)
            for q, (case, k) in enumerate(members):
                for t in range(SAMPLES):
                    f = q * SAMPLES + t
                    cost_ref, strings_ref, status_ref, _ = _ref(case, k, seeds[f])[0]
                    lo, hi = int(offsets[f]), int(offsets[f]) + int(lengths[f])
                    got = tuple(buf[lo:hi].tobytes().decode() for buf in bufs)
                    assert int(status[f]) == 0 and status_ref == "ok", (case, k, t)
                    assert int(costs[q]) == cost_ref and got == strings_ref, (case, k, t)
    finally:
        eng.close()
