"""Guard bands on every device and pinned buffer: where else do the kernels write?

Every other GPU test checks what a kernel writes inside its buffers, bit-exact against the oracle; none checks
what it writes outside them, and each buffer is a separate hipMalloc, so a store one row past the end lands in
allocator slack or in the stale part of a reused buffer, silently.  Under the context option GA_GUARD_BYTES the
engine allocates every DevBuf / PinBuf with a pattern in front of and behind the payload -- the rear guard at the
end of the last REQUEST, not of the capacity -- and every entry that ran kernels ends with a check of them
(GA_E_GUARD, an EngineError here).  Each case below runs an existing parity runner under that option and then
asserts a clean report that lists, guarded and with non-zero payloads, the buffers its path must have used, so
that no case passes without having been guarded.  test_poke_is_reported shows that the check sees a changed
guard byte (a host-side copy into the guard: nothing faults).

Modes: "guard" (GA_GUARD_BYTES=4096: 8x the one overrun the project has had, 4x the widest store of a wave,
64 lanes x 16 B), and "poison-a5" / "poison-ff" (GA_GUARD_POISON=1 under two patterns: every payload starts as the
pattern too, so memory a kernel reads without anyone having written it holds hostile values, not zeros).

The edge sweep of the recompute walk.  The engine takes the recompute walk from 256 x 256 cells up only
(ga_walk_plan.h rc_eligible: below that, degenerate walks read cells no block recomputes), whatever GA_RC says, so
the sweep's rows and columns sit on that floor: m = 256 + {1, 17, 48, 63, 64, 65, 130} (the residues mod 64 of
1, 17, 48, 63, 64, 65, 130: one row into a block, partial 16-row chunks, a block's last row, whole blocks) and
n = 256 and the three columns around the first multiple of the stripe width 64 TD past 256, and 17 past the
multiple two stripes on.  RC_DECLINED lists the shapes the planner declines: none (ga_host_selftest.cpp plans
every one of them on the CPU).  The lane fills below the recompute walk have no floor and run at m = 1 .. 130.
The lane fill has no traceback-word variant at 8 columns per lane (register budget, ga_plan.h lane_geometry), so
the words + walk sweep covers 1, 2 and 4.
"""
import functools
import random

import numpy as np
import pytest

import tests.test_gpu_batch_align as BA  # (the runners below come from the parity files, unchanged)
import tests.test_gpu_batch_rng as BR
import tests.test_gpu_general_costs as GC
import tests.test_gpu_lane as LN
import tests.test_gpu_rc as RC
from tests import general_costs as gc
from tests.conftest import set_knob, splitmix_seq

pytestmark = pytest.mark.gpu

G = 4096
MODES = ["guard", "poison-a5", "poison-ff"]
DNA = RC.DNA


# ---------------------------------------------------------------- guard mode around the existing runners
class Guard:
    """Guard mode for the engines a test creates from here on, and their reports: a runner's own engine just before it
    closes it, the process-wide engines (GlobalAligner's) on request."""

    def __init__(self, monkeypatch, mode):
        from globalign_amd import _native
        self.native = _native
        self.fill = {"guard": 0xA5, "poison-a5": 0xA5, "poison-ff": 0xFF}[mode]
        self.poison = mode != "guard"
        set_knob(monkeypatch, "GA_GUARD_BYTES", G)
        if self.poison:
            set_knob(monkeypatch, "GA_GUARD_POISON", 1)
            set_knob(monkeypatch, "GA_GUARD_FILL", self.fill)
        self.reports = []
        init, close = _native.Engine.__init__, _native.Engine.close

        def owned_init(eng, *args, **kw):
            init(eng, *args, **kw)
            eng._guard_owner = self

        def reporting_close(eng):
            # (an engine of an earlier test, dropped from the process-wide cache only now, is not this test's)
            if getattr(eng, "_h", None) and getattr(eng, "_guard_owner", None) is self:
                self.reports.append(eng.guard_report())
            close(eng)

        monkeypatch.setattr(_native.Engine, "__init__", owned_init)
        monkeypatch.setattr(_native.Engine, "close", reporting_close)

    def clean(self, *must, shared=False):
        """Every engine's report is clean, and their buffers include `must`, guarded and with a non-zero payload."""
        reports = list(self.reports)
        if shared:  # the cached engines made under the options as they are now
            fp = self.native.knob_fingerprint()
            reports += [e.guard_report() for k, e in list(self.native._default.items())
                        if k[2] == fp and getattr(e, "_guard_owner", None) is self]
        assert reports, "no engine ran under guard mode"
        seen = {}
        for r in reports:
            assert r["guard_bytes"] == G and r["fill"] == self.fill and r["poison"] == self.poison, r
            assert r["violations"] == [], r["violations"]
            for b in r["buffers"]:
                if b["guarded"]:
                    seen[b["name"]] = max(seen.get(b["name"], 0), b["payload"])
        missing = [name for name in must if seen.get(name, 0) <= 0]
        assert not missing, (missing, sorted(seen.items()))
        self.reports.clear()
        return seen


@pytest.fixture(params=MODES)
def guard(request, monkeypatch):
    return Guard(monkeypatch, request.param)


FILL_BUFS = ("fb.hand", "fb.flags", "fb.out_last", "fb.top", "fb.left", "fb.GVp", "fb.GHp", "fb.meta", "a", "b", "qp")
WALK_BUFS = ("rng", "result")
RC_BUFS = ("colck", "stck", "rc_tb", "rc_flags", "rc_own", "rc_pos", "qprof", "rc_ops_pin", "rc_ops_prog", "res_pin", "up_pin")


# ---------------------------------------------------------------- the check sees a changed guard byte
def _dna_tables(s1, s2):
    from globalign_amd import _native
    from globalign_amd.scoring import validate_and_transform_args
    _, _, _, cmat, _, goc, _ = validate_and_transform_args(None, None, s1[:64], s2[:64], **DNA)
    return _native.CostTables(cmat, goc)


def test_poke_is_reported(monkeypatch):
    """A byte changed from the host in the front and in the rear guard, at the guard's first and last byte, of a
    checkpoint buffer, a fill's traceback words, the batch kernel's traceback scratch and a pinned buffer: the report
    names exactly that buffer, side, offset and count; the next engine call fails with GA_E_GUARD and the same text;
    that check re-lays the guard, and the context is clean and usable again."""
    from globalign_amd import _native
    set_knob(monkeypatch, "GA_GUARD_BYTES", G)
    set_knob(monkeypatch, "GA_RC", 1)
    s1, s2 = splitmix_seq(300, 1, "dna"), splitmix_seq(449, 2, "dna")
    tables = _dna_tables(s1, s2)
    cases = gc.batch_cases(gc.BATCH_ALIGN_SHAPES[:6], gc.G3)
    btables, codes, chars, seq_off, pa, pb = GC._batch_inputs(cases)
    eng = _native.Engine(0)
    try:
        eng.batch_align(codes, seq_off, pa, pb, btables, list(range(len(cases))), chars)
        eng.load(tables.codes(s1), tables.codes(s2), tables)
        eng.align(GC._mt(1), s1, s2)
        assert eng.fill_kind()[0] == "rc"
        cost = eng.fill(traceback=True)[0]
        rep = eng.guard_report()
        assert rep["violations"] == [] and rep["guard_bytes"] == G and rep["fill"] == 0xA5 and not rep["poison"]
        payload = {b["name"]: b["payload"] for b in rep["buffers"] if b["guarded"]}
        for name in ("colck", "fb.tb", "bt_tb", "rc_ops_pin"):
            assert payload.get(name, 0) > 0, (name, payload)
            for side in ("front", "rear"):
                for at, count in ((0, 1), (G - 1, 1), (100, 7)):
                    eng.guard_poke(name, side, at, count)
                    first = at - G if side == "front" else payload[name] + at
                    want = dict(name=name, side=side, offset=first, last=first + count - 1, changed=count,
                                payload=payload[name])
                    assert eng.guard_report()["violations"] == [want]
                    with pytest.raises(_native.EngineError) as err:
                        eng.fill(traceback=False)
                    text = f"{name} {side} {first:+d} n={count} last={first + count - 1:+d} payload={payload[name]}"
                    assert f"error {_native.GA_E_GUARD}:" in str(err.value) and text in str(err.value), str(err.value)
                    assert eng.guard_report()["violations"] == []
                    assert eng.fill(traceback=False)[0] == cost
        # the poke cannot leave the guard, and needs an allocated, guarded buffer
        for bad in (("colck", "rear", G, 1), ("colck", "rear", G - 1, 2), ("colck", "front", -1, 1), ("colck", "rear", 0, 0),
                    ("no_such", "rear", 0, 1), ("link", "rear", 0, 1), ("chain_io", "front", 0, 1)):
            with pytest.raises(ValueError):
                eng.guard_poke(*bad)
        assert eng.guard_report()["violations"] == []
    finally:
        eng.close()


def test_guard_options_are_checked():
    """GA_GUARD_BYTES is 0 or a multiple of 256 up to 1 MiB, GA_GUARD_FILL a byte, GA_GUARD_POISON needs guards; the
    debug entries need guard mode; and none of it is read from the environment."""
    import os
    from globalign_amd import _native
    for opts in ({"GA_GUARD_BYTES": 100}, {"GA_GUARD_BYTES": 4097}, {"GA_GUARD_BYTES": -256}, {"GA_GUARD_BYTES": 2 ** 20 + 256},
                 {"GA_GUARD_BYTES": "4k"}, {"GA_GUARD_BYTES": 256, "GA_GUARD_FILL": 256}, {"GA_GUARD_POISON": 1},
                 {"GA_GUARD_BYTES": 256, "GA_GUARD_POISON": 2}):
        with pytest.raises(ValueError):
            _native.Engine(0, options=opts)
    os.environ["GA_GUARD_BYTES"] = "100"  # not a shipped knob: ignored, not refused
    try:
        eng = _native.Engine(0, options={"GA_GUARD_BYTES": 0})
    finally:
        del os.environ["GA_GUARD_BYTES"]
    try:
        with pytest.raises(_native.EngineError):
            eng.guard_report()
        with pytest.raises(_native.EngineError):
            eng.guard_poke("colck", "rear", 0, 1)
    finally:
        eng.close()
    eng = _native.Engine(0, options={"GA_GUARD_BYTES": 2 ** 20, "GA_GUARD_FILL": "0x3c", "GA_GUARD_POISON": 1})
    try:
        rep = eng.guard_report()
        assert (rep["guard_bytes"], rep["fill"], rep["poison"], rep["violations"], rep["buffers"]) == (2 ** 20, 0x3c, True, [], [])
    finally:
        eng.close()


# ---------------------------------------------------------------- (a) edge sweep of the lane-family fills
TDS = (1, 2, 4, 8)
RC_FLOOR = 256
RC_ROWS = [RC_FLOOR + r for r in (1, 17, 48, 63, 64, 65, 130)]
LANE_ROWS = [1, 17, 48, 63, 64, 65, 130]


def rc_cols(td):
    w = 64 * td
    k = -(-(RC_FLOOR + 1) // w)  # the first multiple of the stripe width with k w - 1 >= 256
    return [RC_FLOOR, k * w - 1, k * w, k * w + 1, (k + 2) * w + 17]


def lane_cols(td):
    w = 64 * td
    return [1, w - 1, w, w + 1, 3 * w + 17]


# (td, m, n, reason) the planner declines for the recompute walk.  Bound, set before any run: at most 10 % of the
# sweep, and no shape with m >= 64 and n >= 64 td.
RC_DECLINED = []


def test_rc_sweep_declines_within_bound():
    sweep = [(td, m, n) for td in TDS for m in RC_ROWS for n in rc_cols(td)]
    assert len(sweep) == 140 and len(RC_DECLINED) <= len(sweep) // 10
    assert not [d for d in RC_DECLINED if d[1] >= 64 and d[2] >= 64 * d[0]]
    assert all(m >= RC_FLOOR and n >= RC_FLOOR for _, m, n in sweep)


_SWEEP_MODES = [(td, mode) for mode in MODES for td in TDS if mode == "guard" or td in (2, 8)]
_SWEEP_IDS = [f"td{td}-{mode}" for td, mode in _SWEEP_MODES]


@pytest.mark.parametrize("m", RC_ROWS)
@pytest.mark.parametrize("td,mode", _SWEEP_MODES, ids=_SWEEP_IDS)
def test_sweep_recompute_walk(monkeypatch, td, mode, m):
    """GA_RC=1 over the full cross of rows and columns: the checkpointing lane fill's first 64 steps, partial stripes
    and rows past m, then the walk over recomputed blocks; cost, strings and random state against the oracle."""
    guard = Guard(monkeypatch, mode)
    for n in rc_cols(td):
        assert (td, m, n) not in [d[:3] for d in RC_DECLINED]
        kind = RC._align(monkeypatch, splitmix_seq(m, 3 * m + td, "dna"), splitmix_seq(n, 5 * n + td, "dna"), DNA,
                         seed=m + n + td, env={"GA_LANE_COLS_PER_LANE": td})
        assert kind[1] == td, (kind, m, n)
        guard.clean(*RC_BUFS, *FILL_BUFS, *WALK_BUFS)


@pytest.mark.parametrize("td,mode", _SWEEP_MODES, ids=_SWEEP_IDS)
def test_sweep_recompute_walk_general_costs(monkeypatch, td, mode):
    """One letter-dependent, asymmetric table (family G) per stripe width, at a block's last row and a partial stripe."""
    guard = Guard(monkeypatch, mode)
    case = gc.G1 + (RC_FLOOR + 63, rc_cols(td)[-1], 5)
    kind = GC._align(monkeypatch, case, seed=td, knobs={"GA_RC": 1, "GA_LANE_COLS_PER_LANE": td}, fill="rc", walk="rc")
    assert kind[1] == td, kind
    guard.clean(*RC_BUFS, *FILL_BUFS, *WALK_BUFS)


def _adjacent(td, m, n):
    """The subset of the lane sweep: m or n next to a multiple of 64 (of the stripe width), and the four extremes."""
    w = 64 * td
    return m in (63, 64, 65) or n in (w - 1, w, w + 1) or (m in (1, 130) and n in (1, 3 * w + 17))


@pytest.mark.parametrize("m", LANE_ROWS)
@pytest.mark.parametrize("td,mode", _SWEEP_MODES, ids=_SWEEP_IDS)
def test_sweep_lane_score(monkeypatch, td, mode, m):
    """GA_FILL_MODE=lane, score only, m = 1 .. 130: rows shorter than the 64-step lane skew, n < 64 TD."""
    guard = Guard(monkeypatch, mode)
    for n in [n for n in lane_cols(td) if _adjacent(td, m, n)]:
        s1, s2 = splitmix_seq(m, 7 * m + td, "dna"), splitmix_seq(n, 11 * n + td, "dna")
        got, cmat, goc = LN._fill(monkeypatch, td, 4, s1, s2, LN.SCORING)
        assert got == LN._oracle_cost(s1, s2, cmat, goc), (td, m, n)
        guard.clean("qprof", *FILL_BUFS)


@pytest.mark.parametrize("td,mode", _SWEEP_MODES, ids=_SWEEP_IDS)
def test_sweep_lane_score_general_costs(monkeypatch, td, mode):
    guard = Guard(monkeypatch, mode)
    case = gc.G2 + (65, 3 * 64 * td + 17, 6)
    knobs = {"GA_FILL_MODE": "lane", "GA_LANE_COLS_PER_LANE": td, "GA_FILL_NWC": 4}
    assert GC._score(monkeypatch, case, knobs, ("lane", td))[0] == GC._oracle_cost(case)
    guard.clean("qprof", *FILL_BUFS)


_WORD_MODES = [(td, mode) for mode in MODES for td in (1, 2, 4) if mode == "guard" or td == 2]


@pytest.mark.parametrize("m", LANE_ROWS)
@pytest.mark.parametrize("td,mode", _WORD_MODES, ids=[f"td{td}-{mode}" for td, mode in _WORD_MODES])
def test_sweep_lane_words_walk(monkeypatch, td, mode, m):
    """The lane fill's traceback words (window rotation into the row scan's layout) + the stored-words walk."""
    guard = Guard(monkeypatch, mode)
    for n in [n for n in lane_cols(td) if _adjacent(td, m, n)]:
        LN._align_lane(monkeypatch, splitmix_seq(m, 13 * m + td, "dna"), splitmix_seq(n, 17 * n + td, "dna"),
                       LN.SCORING, seed=m ^ n ^ td, td=td)
        guard.clean("fb.tb", "qprof", "ops", *FILL_BUFS, *WALK_BUFS)


@pytest.mark.parametrize("td,mode", _WORD_MODES, ids=[f"td{td}-{mode}" for td, mode in _WORD_MODES])
def test_sweep_lane_words_walk_general_costs(monkeypatch, td, mode):
    guard = Guard(monkeypatch, mode)
    case = gc.G2 + (65, 3 * 64 * td + 17, 5)
    knobs = {"GA_FILL_MODE": "lane", "GA_LANE_COLS_PER_LANE": td, "GA_FILL_NWC": 4}
    GC._align(monkeypatch, case, seed=td, knobs=knobs, fill=("lane", td), walk="stored")
    guard.clean("fb.tb", "qprof", "ops", *FILL_BUFS, *WALK_BUFS)


# ---------------------------------------------------------------- (b) one smallest case per remaining kernel path
BOUNDARY_BUFS = ("fb.bnd_row", "fb.bnd_col", "fb.bscr")


@pytest.mark.parametrize("custom", [False, True], ids=["reference", "caller"])
def test_boundary_kernels(monkeypatch, guard, custom):
    """The boundary pass (make_dp_array) and caller-supplied row-0 / column-0 triples, every cell."""
    GC._full_cells(monkeypatch, gc.FULL_CELLS[0], None, custom=custom)
    guard.clean("full", *BOUNDARY_BUFS, *FILL_BUFS)


@pytest.mark.parametrize("t", [None, 2, 8])
def test_row_scan_every_cell(monkeypatch, guard, t):
    case = gc.G1 + (70, 130, 6)
    assert case in gc.FULL_CELLS
    GC._full_cells(monkeypatch, case, t)
    guard.clean("full", *BOUNDARY_BUFS, *FILL_BUFS)


@pytest.mark.parametrize("o", [3, 20, 300])
def test_row_scan_walk_word_widths(monkeypatch, guard, o):
    case = gc.G1 + (65, 130, o)
    assert case in gc.ROW_WALK
    GC._align(monkeypatch, case, seed=o, knobs={}, fill="row", walk="stored")
    guard.clean("fb.tb", "ops", *FILL_BUFS, *WALK_BUFS)


@pytest.mark.parametrize("case", gc.DIAG, ids=GC._ids(gc.DIAG))
def test_anti_diagonal_fill(monkeypatch, guard, case):
    assert GC._score(monkeypatch, case, {"GA_FILL_MODE": "diag", "GA_DIAG_COLS_PER_LANE": 1}, ("diag", 1))[0] == GC._oracle_cost(case)
    guard.clean(*FILL_BUFS)


@pytest.mark.parametrize("env", [{"GA_LANE_ASM": 0}, {"GA_LANE_DIRECT": 1}, {"GA_LANE_LEAN0": 0}], ids=["asm0", "direct1", "lean0-0"])
def test_lane_handover_variants(monkeypatch, guard, env):
    knobs = dict(env, GA_FILL_MODE="lane", GA_LANE_COLS_PER_LANE=2, GA_FILL_NWC=4)
    assert GC._score(monkeypatch, gc.LANE_HANDOVER, knobs, ("lane", 2))[0] == GC._oracle_cost(gc.LANE_HANDOVER)
    guard.clean("qprof", *FILL_BUFS)


@pytest.mark.parametrize("band_rows", [16, 64])
def test_banded_traceback(monkeypatch, guard, band_rows):
    case = gc.G3 + (300, 500, 5)
    assert (case, band_rows) in gc.BANDED
    GC._align(monkeypatch, case, seed=band_rows, knobs={"GA_TB_BAND_ROWS": band_rows}, walk="stored")
    guard.clean("ckpt", "fb.tb", "ops", *FILL_BUFS, *WALK_BUFS)


@pytest.mark.parametrize("mode,chain", [("lane", 0), ("row", 0), ("lane", 1)], ids=["lane", "row", "lane-chain"])
def test_pipeline(monkeypatch, guard, mode, chain):
    """align_many of 900 x 1000, count 3, under both pipeline fill kernels and with the walks chained in one launch."""
    case = gc.G1 + (900, 1000, 5)
    assert case in gc.PIPELINE
    set_knob(monkeypatch, "GA_PIPE_CHAIN", chain)
    GC.test_pipeline_align_many(monkeypatch, case, mode)
    slots = [f"pipe{s}.{name}" for s in (0, 1) for name in ("fb.tb", "fb.hand", "fb.flags", "fb.out_last", "fb.top", "fb.left")]
    guard.clean(*slots, "pipe_pin", *(("chain_tab", "chain_ctl", "chain_io") if chain else ("pipe0.ops", "pipe0.rng", "pipe0.result")))


BATCH_BUFS = ("bt_codes", "bt_items", "bt_sub", "bt_gh", "bt_gv", "bt_ticket", "bt_out")


@pytest.mark.parametrize("fam", [gc.G3, gc.W2], ids=["G", "W"])
def test_batch_fill_kernel(guard, fam):
    GC.test_batch_costs(fam)
    guard.clean("bt_scratch", *BATCH_BUFS)


@pytest.mark.parametrize("fam", [gc.G3, gc.W2], ids=["G", "W"])
def test_batch_align_kernel(guard, fam):
    GC.test_batch_align(fam)
    guard.clean("bt_witems", "bt_rng", "bt_ops", "bt_walk", "bt_tb", *BATCH_BUFS)


def test_batch_rng_kernel(monkeypatch, guard):
    """The pairs' tie-break tables made on the device: the 60 edge pairs of test_gpu_batch_align through align_pairs,
    and the tables alone at one dispatch, around a 624-word block's end (19.5 dispatches) and over many blocks."""
    import globalign_amd
    set_knob(monkeypatch, "GA_BATCH_RNG", "device")
    set_knob(monkeypatch, "GA_BATCH_RNG_DEVICE_MAX_STEPS", 8192)
    BA._check_pairs(globalign_amd, BA.DNA, BA._edge_pairs(random.Random(11), 60), 1000)
    eng = guard.native.default_engine(0)
    assert eng.batch_align_info()["device_items"] == 60 and not eng.batch_align_info()["fell_back"]
    steps = [1, 19, 20, 21, 700]
    seeds = [0, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1]
    tab, off, status = eng.debug_pair_tables(seeds, steps, rng_tables="device")
    assert status.tolist() == [0] * 5 and eng.batch_align_info()["device_items"] == 5
    for k, (s, n) in enumerate(zip(seeds, steps)):
        assert np.array_equal(tab[off[k]:off[k + 1]], BR.cpython_table(s, n)), (s, n)
    guard.clean("bt_ritems", "bt_rstatus", "bt_rbase", "bt_rng", "bt_tb", *BATCH_BUFS, shared=True)


@pytest.mark.parametrize("rc", [False, True], ids=["words", "rc"])
def test_slabs_in_process(monkeypatch, guard, rc):
    """Three column slabs (1500 x 3 * 512 + 77) on one GPU, linked device to device.  `link` is outside guard mode."""
    GC.test_slabs_in_process(monkeypatch, rc)
    seen = guard.clean("halo_in", "prog", "fb.hand", *(("colck", "stck", "rc_tb") if rc else ("fb.tb",)))
    assert "link" not in seen


def test_protein_row_scan(monkeypatch, guard):
    """BLOSUM62 (K = 25, two-byte words) through the default call of a small problem: row scan + stored words."""
    from globalign_amd import _native
    from globalign_amd.scoring import validate_and_transform_args
    from oracle import core, transform
    from tests.conftest import load_matrix
    kw = dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)
    s1, s2 = splitmix_seq(600, 3, "protein"), splitmix_seq(700, 4, "protein")
    a1, a2, smat, cmat, gos, goc = transform.settings(dict(kw, seq_1=s1, seq_2=s2), blosum=load_matrix("BLOSUM62"))
    mt = GC._mt(3)
    ref = core.align(a1, a2, cmat, goc, mt)
    _, _, _, cmat2, _, goc2, _ = validate_and_transform_args(None, None, s1[:64], s2[:64], **kw)
    tables = _native.CostTables(cmat2, goc2)
    eng = _native.Engine(0)
    try:
        eng.load(tables.codes(a1), tables.codes(a2), tables)
        cost, strings, status, mt_after = eng.align(mt, a1, a2)
        kind, walk = eng.fill_kind(), eng.walk_kind()
    finally:
        eng.close()
    assert kind[0] == "row" and walk == "stored", (kind, walk)
    assert status == 0 and int(cost) == ref["cost"] and tuple(strings) == tuple(ref["strings"])
    assert np.asarray(mt_after, dtype=np.uint32).tolist() == np.asarray(ref["mt_out"], dtype=np.uint32).tolist()
    guard.clean("fb.tb", *FILL_BUFS, *WALK_BUFS)


def test_protein_recompute_walk(monkeypatch, guard):
    """test_gpu_rc's BLOSUM62 shape halved (600 x 700: still above the recompute walk's floor)."""
    kw = dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)
    RC._align(monkeypatch, splitmix_seq(600, 3, "protein"), splitmix_seq(700, 4, "protein"), kw, seed=3, protein=True)
    guard.clean(*RC_BUFS, *FILL_BUFS, *WALK_BUFS)


# ---------------------------------------------------------------- (c) reuse: large, small, large on one engine
@functools.lru_cache(maxsize=None)
def _dna_reference(m, n, seed):
    from oracle import core, transform
    s1, s2 = splitmix_seq(m, 100 + m, "dna"), splitmix_seq(n, 200 + n, "dna")
    a1, a2, smat, cmat, gos, goc = transform.settings(dict(DNA, seq_1=s1, seq_2=s2))
    ref = core.align(a1, a2, cmat, goc, GC._mt(seed))
    return s1, s2, ref["cost"], tuple(ref["strings"]), tuple(np.asarray(ref["mt_out"], dtype=np.uint32).tolist())


def _payloads(eng):
    rep = eng.guard_report()
    assert rep["violations"] == [], rep["violations"]
    return {b["name"]: b["payload"] for b in rep["buffers"] if b["guarded"]}


def test_reuse_recompute_walk(monkeypatch, guard):
    """2049 x 700, 65 x 129 (below the recompute walk's floor: the stored-words call, in the same context), 2049 x 700:
    the guards follow each request down and up again -- the rear guard sits at the request's end, not at the
    capacity's -- and the checkpoint buffers the small call does not use stay as the large one left them."""
    from globalign_amd import _native
    set_knob(monkeypatch, "GA_RC", 1)
    eng = _native.Engine(0)
    try:
        sizes = []
        for step, (m, n) in enumerate([(2049, 700), (65, 129), (2049, 700)]):
            s1, s2, cost_ref, strings_ref, mt_ref = _dna_reference(m, n, 7)
            tables = _dna_tables(s1, s2)
            eng.load(tables.codes(s1), tables.codes(s2), tables)
            cost, strings, status, mt_after = eng.align(GC._mt(7), s1, s2)
            assert eng.fill_kind()[0] == ("rc" if min(m, n) >= RC_FLOOR else "row"), (step, eng.fill_kind())
            assert status == 0 and int(cost) == cost_ref and tuple(strings) == strings_ref
            assert tuple(np.asarray(mt_after, dtype=np.uint32).tolist()) == mt_ref
            p = _payloads(eng)
            assert (p["a"], p["b"], p["ops"], p["rng"]) == (m, n, m + n + 1024, 4 * (m + n + 2 + 64)), (step, p)
            assert (p["fb.bnd_col"], p["fb.GVp"], p["fb.left"], p["fb.top"]) == (12 * (m + 1), 4 * (m + 1), 8 * (m + 1), 8 * (n + 1))
            sizes.append(p)
        # (the small call's traceback words are the one buffer the first large call had not allocated)
        assert set(sizes[2]) - set(sizes[0]) == {"fb.tb"} and {k: sizes[2][k] for k in sizes[0]} == sizes[0]
        for name in ("colck", "stck", "rc_tb", "rc_flags", "qprof"):
            assert sizes[0][name] > 0 and sizes[1][name] == sizes[0][name], name
        assert sizes[1]["fb.tb"] > 0
    finally:
        eng.close()
    guard.clean(*RC_BUFS)


def test_reuse_align_pairs(guard):
    """ga_batch_align with 21 pairs up to 513 x 513, then two short pairs, then the 21 again."""
    from globalign_amd import _native
    large = gc.batch_cases(gc.BATCH_ALIGN_SHAPES[:21], gc.G3)
    small = gc.batch_cases([(2, 2), (65, 129)], gc.G3)
    eng = _native.Engine(0)
    try:
        sizes = []
        for cases in (large, small, large):
            tables, codes, chars, seq_off, pa, pb = GC._batch_inputs(cases)
            seeds = [3 + k for k in range(len(cases))]
            costs, status, lengths, offsets, bufs = eng.batch_align(codes, seq_off, pa, pb, tables, seeds, chars)
            for k, (case, seed) in enumerate(zip(cases, seeds)):
                cmat, s1, s2, o = GC._problem(case)
                r = _pair_reference(case, seed)
                lo, hi = int(offsets[k]), int(offsets[k]) + int(lengths[k])
                assert int(costs[k]) == r[0] and int(status[k]) == 0 and r[2] == "ok", (case, seed)
                assert tuple(buf[lo:hi].tobytes().decode() for buf in bufs) == r[1], (case, seed)
            p = _payloads(eng)
            assert (p["bt_codes"], p["bt_out"], p["bt_walk"]) == (codes.size, 8 * len(cases), 32 * len(cases)), p
            sizes.append(p)
        assert sizes[0] == sizes[2] and sizes[1]["bt_rng"] < sizes[0]["bt_rng"] and sizes[1]["bt_ops"] < sizes[0]["bt_ops"]
    finally:
        eng.close()
    guard.clean("bt_tb", "bt_rng", "bt_ops", *BATCH_BUFS)


@functools.lru_cache(maxsize=None)
def _pair_reference(case, seed):
    from oracle import core
    cmat, s1, s2, o = GC._problem(case)
    r = core.align(s1, s2, cmat, o, GC._mt(seed))
    return r["cost"], tuple(r["strings"]), r["status"]


def test_reuse_pipeline(guard):
    """align_many, count 3, of 900 x 1000, then 65 x 130, then 900 x 1000 in one context: every slot's buffers shrink
    and grow with the problem."""
    from globalign_amd import _native
    eng = _native.Engine(0)
    try:
        sizes = []
        for case in (gc.G1 + (900, 1000, 5), gc.G1 + (65, 130, 3), gc.G1 + (900, 1000, 5)):
            m, n = case[2], case[3]
            tables, s1, s2 = GC._tables(case)
            ref = GC._ref_chain(case, 9, 3)
            eng.load(tables.codes(s1), tables.codes(s2), tables)
            runs, mt_after = eng.align_many(GC._mt(9), s1, s2, 3)
            for (cost, strings, status), (cost_ref, strings_ref, status_ref, _) in zip(runs, ref):
                assert status == 0 and status_ref == "ok" and cost == cost_ref and tuple(strings) == strings_ref
            assert tuple(np.asarray(mt_after, dtype=np.uint32).tolist()) == ref[-1][3]
            p = _payloads(eng)
            for s in (0, 1):
                assert (p[f"pipe{s}.ops"], p[f"pipe{s}.rng"], p[f"pipe{s}.tab_pin"]) == (m + n + 1024, 4 * (m + n + 1 + 64), 4 * (m + n + 1)), (s, p)
                assert p[f"pipe{s}.fb.left"] == 8 * (m + 1) and p[f"pipe{s}.fb.tb"] > 0
            sizes.append(p)
        assert sizes[0] == sizes[2] and sizes[1]["pipe0.fb.tb"] < sizes[0]["pipe0.fb.tb"]
    finally:
        eng.close()
    guard.clean("pipe0.fb.tb", "pipe1.fb.tb", "pipe_pin")
