"""Long gap runs, seam crossings, edge arrivals, corridors and dispatch counts on every walker.

tests/test_gpu_tie_classes.py covers what a walked cell can decide; the case lists of tests/path_geometry.py cover
where the path goes: gap runs wider than the walk's tile torus and the recompute walk's candidate window (W1), runs
that start and end on tile seams (W2), moves through tile corners (W3), every way of arriving at row 0 or column 0
(W4), corridors within 25 cells of an edge (W5), dispatch counts at the level words' and the ring's block ends (W6),
band tops crossed in a run and at the first columns (W7) and slab edges crossed in either level (W8).
tests/test_path_geometry_cpu.py proves on the CPU oracle that the lists reach those classes at every word width.
Here each list goes through every traceback path, bit-exact against oracle.core: cost, the three strings, status
and all 625 MT words where the path returns them.  One test per (path, width) runs its whole list on one engine.

The stored-words walk waits for a tile without a bound, so a liveness fault on a planted path would show as a hang:
run this module under a time limit of its own."""
import functools

import numpy as np
import pytest

from tests import gpu_parity as gp
from tests import path_geometry as pg
from tests.conftest import set_knob

pytestmark = pytest.mark.gpu

WIDTHS = pg.WIDTHS
SAMPLES = 3
RUN_LISTS = ("RUNS", "RC_RUNS")


@functools.lru_cache(maxsize=None)
def _problem(case):
    return pg.problem(case)


@functools.lru_cache(maxsize=None)
def _ref(case, seed, count=1):
    """`count` chained oracle alignments of a case from random.seed(seed)."""
    return gp.ref_chain(_problem(case), seed, count)


def _items(path, width, int8=False, names=None):
    """[(problem, seed, oracle result)] of a path's list at a width."""
    out = []
    for case in pg.path_cases(path, width, int8, names):
        assert pg.tb_word_bytes(case[0][1]) == width
        out.append((_problem(case), pg.case_seed(case), _ref(case, pg.case_seed(case))[0]))
    assert out
    return out


# ---------------------------------------------------------------- single calls
@pytest.mark.parametrize("width", WIDTHS)
def test_stored_walk_long_runs(monkeypatch, width):
    """W1 on the stored-words walk alone (need_tile, the loaders' skip_corners): the runs of five seams and more, and
    the recompute list's 700-column and 2100-row runs."""
    gp.align_cases(monkeypatch, _items("single", width, names=RUN_LISTS), {}, fill="row", walk="stored")


@pytest.mark.parametrize("width", WIDTHS)
def test_row_scan_stored_walk(monkeypatch, width):
    gp.align_cases(monkeypatch, _items("single", width), {}, fill="row", walk="stored")


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("td", [1, 2])
def test_lane_words_stored_walk(monkeypatch, td, width):
    knobs = {"GA_FILL_MODE": "lane", "GA_LANE_COLS_PER_LANE": td}
    gp.align_cases(monkeypatch, _items("single", width, int8=True), knobs, fill=("lane", td), walk="stored")


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("td", [1, 2])
def test_recompute_walk(monkeypatch, td, width):
    """The word walk over recomputed blocks; the list's runs leave the candidate window (7 stripes left, 31 block
    rows up) at 1 column per lane."""
    knobs = {"GA_RC": 1, "GA_LANE_COLS_PER_LANE": td, "GA_RC_JUMP": 0}
    kinds = gp.align_cases(monkeypatch, _items("rc", width, int8=True), knobs, fill="rc", walk="rc")
    assert all(kind[0] == "rc" for kind in kinds)


@pytest.mark.parametrize("width", WIDTHS)
def test_recompute_walk_one_server(monkeypatch, width):
    """One serving workgroup and the smallest window (the walker's own 2 x 2 blocks) on the W1 runs: every block of a
    long run is asked for, none is ready ahead."""
    knobs = {"GA_RC": 1, "GA_LANE_COLS_PER_LANE": 1, "GA_RC_JUMP": 0, "GA_RC_SERVERS": 1, "GA_RC_WIN": 4}
    kinds = gp.align_cases(monkeypatch, _items("rc", width, int8=True, names=RUN_LISTS), knobs, fill="rc", walk="rc")
    assert all(kind[0] == "rc" for kind in kinds)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("band_rows", pg.BAND_ROWS)
def test_banded_refills(monkeypatch, band_rows, width):
    """banded_align: W7 (band tops in a run, entry columns 1, 2, 63, 64, 65, walks ending in a lower band) with W1
    and W4.  No fill kind is asserted (fill_kind() does not tell a banded traceback from a whole one): every case has
    m >= 2 * band_rows, which forces the bands."""
    items = _items("banded", width)
    assert all(len(p[1]) >= 2 * band_rows for p, _, _ in items)
    gp.align_cases(monkeypatch, items, {"GA_TB_BAND_ROWS": band_rows}, walk="stored")


# ---------------------------------------------------------------- pipeline
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mode,chain", [("lane", None), ("row", None), ("lane", 1)], ids=["lane", "row", "lane-chain"])
def test_pipeline_align_many(monkeypatch, mode, chain, width):
    """Engine.align_many, three alignments chained through the random state (GA_PIPE_CHAIN=1: walk_body's ring
    path), over W1, W4, W5 and W6."""
    from globalign_amd import _native
    set_knob(monkeypatch, "GA_PIPE_MODE", mode)
    if chain is not None:
        set_knob(monkeypatch, "GA_PIPE_CHAIN", chain)
    want = ("lane", 4 if width == 1 else 2) if mode == "lane" else ("row",)
    eng = _native.Engine(0)
    try:
        for q, case in enumerate(pg.path_cases("pipe", width, int8=mode == "lane")):
            seed = pg.case_seed(case)
            problem, ref = _problem(case), _ref(case, seed, 3)
            tabs, s1, s2 = gp.tables(problem)
            eng.load(tabs.codes(s1), tabs.codes(s2), tabs)
            runs, mt_after = eng.align_many(gp.mt(seed), s1, s2, 3)
            kind = eng.fill_kind()
            assert kind[:len(want)] == want, (q, case, kind)
            assert len(runs) == 3
            for (cost, strings, status), (cost_ref, strings_ref, status_ref, _) in zip(runs, ref):
                assert status == 0 and status_ref == "ok", (q, case)
                assert cost == cost_ref and tuple(strings) == strings_ref, (q, case)
            assert tuple(np.asarray(mt_after, dtype=np.uint32).tolist()) == ref[-1][3], (q, case)
    finally:
        eng.close()


# ---------------------------------------------------------------- batches (one table and gap open cost per call)
def _groups(width):
    """The batch list of a width by cost setting: {(kind, o): [case]}, in list order."""
    out = {}
    for case in pg.path_cases("batch", width):
        out.setdefault(case[0], []).append(case)
    return out


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("route", ["host", "device"])
def test_batch_align(monkeypatch, route, width):
    """batch_align_kernel and the batch walker (groups of up to 7 steps over an 8 x 8 window clamped at row 1 and
    column 1), every case of a cost setting in one batch; tie-break entries made by the host and on the device."""
    from globalign_amd import _native
    set_knob(monkeypatch, "GA_BATCH_RNG_DEVICE_MAX_STEPS", 8192)
    eng = _native.Engine(0)
    try:
        for key, members in _groups(width).items():
            problems = [_problem(c) for c in members]
            seeds = [pg.case_seed(c) for c in members]
            tabs, codes, chars, seq_off, pa, pb = gp.batch_inputs(problems)
            costs, status, lengths, offsets, bufs = eng.batch_align(codes, seq_off, pa, pb, tabs, seeds, chars,
                                                                    rng_tables=route)
            info = eng.batch_align_info()
            P = len(members)
            assert (info["device_items"], info["host_items"], info["fell_back"]) == \
                ((P, 0, False) if route == "device" else (0, P, False)), (key, info)
            for q, (case, seed) in enumerate(zip(members, seeds)):
                cost_ref, strings_ref, status_ref, _ = _ref(case, seed)[0]
                lo, hi = int(offsets[q]), int(offsets[q]) + int(lengths[q])
                got = tuple(buf[lo:hi].tobytes().decode() for buf in bufs)
                assert int(status[q]) == 0 and status_ref == "ok", case
                assert int(costs[q]) == cost_ref and got == strings_ref, case
    finally:
        eng.close()


@pytest.mark.parametrize("width", WIDTHS)
def test_batch_sample(width):
    """batch_words_kernel + batch_walks_kernel: three seeded walks of every pair from one fill of it."""
    from globalign_amd import _native
    eng = _native.Engine(0)
    try:
        for key, members in _groups(width).items():
            problems = [_problem(c) for c in members]
            P = len(members)
            seeds = [pg.case_seed(c) + t for c in members for t in range(SAMPLES)]
            tabs, codes, chars, seq_off, pa, pb = gp.batch_inputs(problems)
            sample_off = np.arange(P + 1, dtype=np.int64) * SAMPLES
            costs, status, lengths, offsets, bufs = eng.batch_sample(codes, seq_off, pa, pb, tabs, sample_off, seeds,
                                                                     chars)
            info = eng.batch_sample_info()
            assert (info["filled_pairs"], info["walk_items"], info["single_fill_pairs"], info["looped_pairs"]) == \
                (P, SAMPLES * P, 0, 0), (key, info)
            for q, case in enumerate(members):
                for t in range(SAMPLES):
                    f = q * SAMPLES + t
                    cost_ref, strings_ref, status_ref, _ = _ref(case, seeds[f])[0]
                    lo, hi = int(offsets[f]), int(offsets[f]) + int(lengths[f])
                    got = tuple(buf[lo:hi].tobytes().decode() for buf in bufs)
                    assert int(status[f]) == 0 and status_ref == "ok", (case, t)
                    assert int(costs[q]) == cost_ref and got == strings_ref, (case, t)
    finally:
        eng.close()


# ---------------------------------------------------------------- slabs in one process
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("rc", [False, True], ids=["stored", "rc"])
def test_slabs_in_process(monkeypatch, rc, width):
    """Three column slabs on one GPU over W8: the walk handed right to left at local column 0 in level 0 and inside a
    level-1 run, a run across the whole middle slab, vertical runs in a slab's first and last column, walks that end
    in the middle and in the right slab.  rc: every slab of at least 256 columns (the recompute walk's floor; m is
    above it in every case) must report the recompute fill."""
    from globalign_amd import distributed
    if rc:
        set_knob(monkeypatch, "GA_RC", 1)
    engines = [distributed.GpuSlabEngine(0) for _ in range(3)]
    try:
        for q, case in enumerate(pg.path_cases("slabs", width)):
            problem, seed = _problem(case), pg.case_seed(case)
            tabs, s1, s2 = gp.tables(problem)
            edges = distributed.slab_bounds(len(s2), 3)
            assert edges == pg.slab_bounds(len(s2)) and len(s1) >= 256
            cost_ref, strings_ref, status_ref, mt_ref = _ref(case, seed)[0]
            cost, strings, status, mt_after = distributed.align_devices([0, 0, 0], s1, s2, tabs.codes(s1),
                                                                        tabs.codes(s2), tabs, gp.mt(seed),
                                                                        engines=engines)
            assert status == 0 and status_ref == "ok", (q, case)
            assert int(cost) == cost_ref and tuple(strings) == strings_ref, (q, case)
            assert tuple(np.asarray(mt_after, dtype=np.uint32).tolist()) == mt_ref, (q, case)
            if rc:
                wide = [k for k in range(3) if edges[k + 1] - edges[k] >= 256]
                assert len(wide) >= 2
                for k in wide:
                    assert engines[k].eng.fill_kind()[0] == "rc", (q, case, k, engines[k].eng.fill_kind())
    finally:
        for e in engines:
            e.eng.close()
