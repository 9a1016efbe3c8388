"""GPU parity under letter-dependent, asymmetric cost tables on every fill and walk path.

Every fill works in a shifted domain (V' = V - GV(i) - GH(j), sub' = sub - gap_v[a] - gap_h[b]); the
shift is invisible under DNA match/mismatch tables, BLOSUM62 or a one-gap-score matrix, where gap_h[a_i] read for
gap_h[b_j], gh and gv swapped, sub read transposed or a prefix sum carried wrongly across a stripe, workgroup, slab,
band, checkpoint or pair boundary all give the same numbers.  Here the tables of tests/general_costs.py (G: general,
int8 profile; W: wide and signed, int16 profile; S: a score matrix file with a gap score per letter, through the
public API) go through each path at the smallest shapes that cross its structure, bit-exact against oracle.core
under the same table: cost, the three strings and all 625 MT words, or every cell where stated.
tests/test_oracle.py::test_general_cost_cases_can_fail shows on the CPU that these cases tell the tables apart.

The lane-skewed fill and the recompute walk are built for an int8 profile (lane_geometry declines
qbytes == 2).  Family W under GA_FILL_MODE=lane / GA_RC=1 must therefore take the row scan / the stored-words walk,
and the cases assert exactly that, so that no case takes another path than the one written down for it."""
import functools
import random

import numpy as np
import pytest

from tests import general_costs as gc
from tests import gpu_parity as gp
from tests.conftest import set_knob

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- shared, cached references
# (the engine calls themselves are tests/gpu_parity.py's, shared with tests/test_gpu_limits.py)
@functools.lru_cache(maxsize=None)
def _problem(case):
    """(costing dict, seq_1, seq_2, gap open cost) of a case."""
    s1, s2 = gc.sequences(case)
    return gc.table(case[0], case[1]), s1, s2, case[4]


_mt = gp.mt


@functools.lru_cache(maxsize=None)
def _ref_chain(case, seed, count=1):
    """`count` consecutive oracle alignments of a case from random.seed(seed): [(cost, strings, status, mt words)]."""
    return gp.ref_chain(_problem(case), seed, count)


def _tables(case):
    cmat = _problem(case)[0]
    tables, s1, s2 = gp.tables(_problem(case))
    assert tables.gap_h.tolist()[:4] == gc.gap_h(cmat) and tables.gap_v.tolist()[:4] == gc.gap_v(cmat)
    return tables, s1, s2


def _int8(case):
    return gc.profile_bytes(_problem(case)[0]) == 1


def _align(monkeypatch, case, seed, knobs, fill=None, walk=None):
    """Engine.align of a case under `knobs` against the oracle: cost, strings, status and every MT word; fill / walk:
    what fill_kind() / walk_kind() must report (fill: a kind, or (kind, columns per lane))."""
    _tables(case)
    return gp.align(monkeypatch, _problem(case), seed, knobs, _ref_chain(case, seed)[0], fill=fill, walk=walk)


def _score(monkeypatch, case, knobs, fill, load_kw=None, problem=None):
    """Engine.fill(traceback=False) under `knobs` -> the cost; fill: the fill_kind() prefix that must have run."""
    return gp.score(monkeypatch, problem or _problem(case), knobs, fill, load_kw)


@functools.lru_cache(maxsize=None)
def _oracle_cost(case):
    cmat, s1, s2, o = _problem(case)
    return gc.oracle_cost(cmat, s1, s2, o)


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


# ---------------------------------------------------------------- every cell (the un-shift of each one), row scan
@functools.lru_cache(maxsize=None)
def _full_reference(case, custom):
    """core.fill_full over the reference's boundary, or (custom) over random caller triples -> (dp, row0, col0)."""
    boundary = None
    if custom:
        m, n = case[2], case[3]
        rng = np.random.default_rng(5)
        row0 = rng.integers(0, 400, size=3 * (n + 1)).astype(np.int64)
        col0 = rng.integers(0, 400, size=3 * (m + 1)).astype(np.int64)
        row0[:3] = col0[:3] = 0
        boundary = (row0, col0)
    return gp.full_reference(_problem(case), boundary)


def _full_cells(monkeypatch, case, t, custom=False):
    _tables(case)
    gp.full_cells(monkeypatch, _problem(case), t, _full_reference(case, custom), custom)


@pytest.mark.parametrize("t", [None, 2, 8])
@pytest.mark.parametrize("case", gc.FULL_CELLS, ids=_ids(gc.FULL_CELLS))
def test_every_cell_row_scan(monkeypatch, case, t):
    """Engine.fill(full=True): all three values of every interior cell, un-shifted by its own GV(i) + GH(j), against
    core.fill_full; two and three stripes with a partial last one, more than one 64-row block."""
    _full_cells(monkeypatch, case, t)


def test_every_cell_custom_boundary(monkeypatch):
    """The same over random caller-supplied row-0 / column-0 triples, wide table."""
    _full_cells(monkeypatch, gc.FULL_CELLS[-1], None, custom=True)


# ---------------------------------------------------------------- row scan + walk, default geometry
@pytest.mark.parametrize("case", gc.ROW_WALK, ids=_ids(gc.ROW_WALK))
def test_row_scan_walk(monkeypatch, case):
    """The default single call of a small problem (row scan with traceback words, stored-words walk) at one-, two-
    and four-byte words."""
    _align(monkeypatch, case, seed=case[2] ^ case[3], knobs={}, fill="row", walk="stored")


# ---------------------------------------------------------------- lane fill
_LANE_SCORE = [(td, nwc, c) for td in gc.LANE_TDS for nwc in (4, 8) for c in gc.lane_score_cases(td)]


@pytest.mark.parametrize("td,nwc,case", _LANE_SCORE, ids=[f"td{t}-nwc{w}-" + _ids([c])[0] for t, w, c in _LANE_SCORE])
def test_lane_score(monkeypatch, td, nwc, case):
    """GA_FILL_MODE=lane at every stripe width and both workgroup sizes: one stripe, n < 64 TD, five stripes and a
    partial sixth (two workgroups of 4), rows shorter than the lane skew.  W (int16 profile): the row scan."""
    knobs = {"GA_FILL_MODE": "lane", "GA_LANE_COLS_PER_LANE": td, "GA_FILL_NWC": nwc}
    fill = ("lane", td) if _int8(case) else ("row",)
    got, kind = _score(monkeypatch, case, knobs, fill)
    assert kind[3] == nwc, kind
    assert got == _oracle_cost(case)


_LANE_WALK = [(td, c) for td in (1, 2, 4) for c in gc.lane_walk_cases(td)]


@pytest.mark.parametrize("td,case", _LANE_WALK, ids=[f"td{t}-" + _ids([c])[0] for t, c in _LANE_WALK])
def test_lane_words_walk(monkeypatch, td, case):
    """The lane fill's traceback words (window rotation into the row scan's layout) + the walk."""
    knobs = {"GA_FILL_MODE": "lane", "GA_LANE_COLS_PER_LANE": td, "GA_FILL_NWC": 4}
    _align(monkeypatch, case, seed=td + case[2], knobs=knobs, fill=("lane", td) if _int8(case) else "row", walk="stored")


@pytest.mark.parametrize("env", [{"GA_LANE_ASM": 0}, {"GA_LANE_DIRECT": 1}, {"GA_LANE_LEAN0": 0}],
                         ids=["asm0", "direct1", "lean0-0"])
def test_lane_handover_variants(monkeypatch, env):
    """The compiler's steps, the direct workgroup hand-off and the masked ramp, over three workgroups at TD 2."""
    knobs = dict(env, GA_FILL_MODE="lane", GA_LANE_COLS_PER_LANE=2, GA_FILL_NWC=4)
    assert _score(monkeypatch, gc.LANE_HANDOVER, knobs, ("lane", 2))[0] == _oracle_cost(gc.LANE_HANDOVER)


def test_lane_lean_ramp_needs_every_prefix(monkeypatch):
    """The lean ramp assumes a uniform row 0 in the shifted domain, h2'(0, j) = min(big - GH(j), 2o) = 2o in EVERY
    column.  With gap costs of mixed sign GH is not monotone: here 2o + GH(35) = 14450 > big = 14070 >= 2o + GH(70),
    so a test of GH(n) alone would turn the lean ramp on over columns whose row-0 values are not uniform; the host
    tests the largest prefix sum.  (A path that enters such a column from row 0 cannot be optimal at this gap open,
    so the final cost alone does not tell the two predicates apart: the case pins that the lane fill of a problem
    with a falling GH stays exact, the predicate itself rests on the reasoning above.)"""
    cmat, s1, s2, o = gc.lean_ramp_case()
    knobs = {"GA_FILL_MODE": "lane", "GA_LANE_COLS_PER_LANE": 1, "GA_FILL_NWC": 4}
    got, _ = _score(monkeypatch, None, knobs, ("lane", 1), problem=(cmat, s1, s2, o))
    assert got == gc.oracle_cost(cmat, s1, s2, o)


# ---------------------------------------------------------------- anti-diagonal fill
@pytest.mark.parametrize("td", [1, 2, 4])
@pytest.mark.parametrize("case", gc.DIAG, ids=_ids(gc.DIAG))
def test_diag_score(monkeypatch, td, case):
    knobs = {"GA_FILL_MODE": "diag", "GA_DIAG_COLS_PER_LANE": td}
    assert _score(monkeypatch, case, knobs, ("diag", td))[0] == _oracle_cost(case)


# ---------------------------------------------------------------- recompute walk
@pytest.mark.parametrize("case,td,every", gc.RC, ids=[_ids([c])[0] + f"-td{t}-every{e}" for c, t, e in gc.RC])
def test_recompute_walk(monkeypatch, case, td, every):
    """GA_RC=1: the checkpointing lane fill (right-edge columns, staircase states) and the walk that recomputes 64-row
    blocks from them, at every stripe width.  W (int16 profile): the recompute walk declines, the stored words run."""
    knobs = {"GA_RC": 1}
    if td is not None:
        knobs["GA_LANE_COLS_PER_LANE"] = td
    if every is not None:
        knobs["GA_RC_EVERY"] = every
    if _int8(case):
        kind = _align(monkeypatch, case, seed=case[2] + case[4], knobs=knobs, fill="rc", walk="rc")
        assert td is None or kind[1] == td, kind
    else:
        _align(monkeypatch, case, seed=case[2] + case[4], knobs=knobs, fill="row", walk="stored")


# ---------------------------------------------------------------- banded traceback
@pytest.mark.parametrize("case,band_rows", gc.BANDED, ids=[_ids([c])[0] + f"-bh{b}" for c, b in gc.BANDED])
def test_banded_traceback(monkeypatch, case, band_rows):
    """Checkpoint rows every band_rows rows, band refills from them over column prefixes, the walk handed on at each
    band top; the tall case's checkpoint pass takes the lane fill."""
    _align(monkeypatch, case, seed=case[3] ^ band_rows, knobs={"GA_TB_BAND_ROWS": band_rows}, walk="stored")


# ---------------------------------------------------------------- pipeline
@pytest.mark.parametrize("mode", ["lane", "row"])
@pytest.mark.parametrize("case", gc.PIPELINE, ids=_ids(gc.PIPELINE))
def test_pipeline_align_many(monkeypatch, case, mode):
    """Engine.align_many, three alignments chained through the random state, under both pipeline fill kernels."""
    from globalign_amd import _native
    set_knob(monkeypatch, "GA_PIPE_MODE", mode)
    tables, s1, s2 = _tables(case)
    ref = _ref_chain(case, 9, 3)
    eng = _native.Engine(0)
    try:
        eng.load(tables.codes(s1), tables.codes(s2), tables)
        runs, mt_after = eng.align_many(_mt(9), s1, s2, 3)
    finally:
        eng.close()
    assert len(runs) == 3
    for (cost, strings, status), (cost_ref, strings_ref, status_ref, _) in zip(runs, ref):
        assert status == 0 and status_ref == "ok"
        assert cost == cost_ref and tuple(strings) == strings_ref
    assert tuple(np.asarray(mt_after, dtype=np.uint32).tolist()) == ref[-1][3]


# ---------------------------------------------------------------- batches
def _batch_inputs(cases):
    """codes / chars / seq_off / pair indices of a batch whose pair k is cases[k] (all under one table)."""
    return gp.batch_inputs([_problem(c) for c in cases])


@pytest.mark.parametrize("fam", [gc.G3, gc.W2], ids=["G", "W"])
def test_batch_costs(fam):
    """Engine.batch_costs: a wave per pair with the pair's own prefix sums and un-shift; lengths 1 to 513 on either
    side, the edge column in LDS (70 x 5000) and in HBM (1100 x 600)."""
    from globalign_amd import _native
    cases = gc.batch_cases(gc.BATCH_COST_SHAPES, fam)
    tables, codes, _, seq_off, pa, pb = _batch_inputs(cases)
    eng = _native.Engine(0)
    try:
        costs = eng.batch_costs(codes, seq_off, pa, pb, tables)
    finally:
        eng.close()
    want = [_oracle_cost(c) for c in cases]
    bad = [(c, int(g), w) for c, g, w in zip(cases, costs, want) if int(g) != w]
    assert not bad, bad[:6]


_BATCH_SEEDS = [0, 5, 5, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1, 2 ** 40]


@pytest.mark.parametrize("fam", [gc.G3, gc.W2], ids=["G", "W"])
def test_batch_align(fam):
    """Engine.batch_align: fill with words and walk by one wave per pair, each pair under a seed of its own (some
    equal, some at and past 2^32): cost, status, strings."""
    from globalign_amd import _native
    from oracle import core
    cases = gc.batch_cases(gc.BATCH_ALIGN_SHAPES, fam)
    seeds = [(_BATCH_SEEDS[k % len(_BATCH_SEEDS)] + (k // len(_BATCH_SEEDS)) * 1000) % 2 ** 64 for k in range(len(cases))]
    tables, codes, chars, seq_off, pa, pb = _batch_inputs(cases)
    eng = _native.Engine(0)
    try:
        costs, status, lengths, offsets, bufs = eng.batch_align(codes, seq_off, pa, pb, tables, seeds, chars)
    finally:
        eng.close()
    bad = []
    for k, (case, seed) in enumerate(zip(cases, seeds)):
        cmat, s1, s2, o = _problem(case)
        r = core.align(s1, s2, cmat, o, _mt(seed))
        lo, hi = int(offsets[k]), int(offsets[k]) + int(lengths[k])
        got = tuple(buf[lo:hi].tobytes().decode() for buf in bufs)
        ok = int(costs[k]) == r["cost"] and int(status[k]) == (0 if r["status"] == "ok" else _native.GA_TB_INDEX_ERROR)
        if ok and r["status"] == "ok":
            ok = got == tuple(r["strings"])
        if not ok:
            bad.append((case, seed, int(costs[k]), r["cost"], int(status[k]), r["status"]))
    assert not bad, bad[:6]


# ---------------------------------------------------------------- slabs in one process
@pytest.mark.parametrize("rc", [False, True], ids=["words", "rc"])
def test_slabs_in_process(monkeypatch, rc):
    """Three column slabs on one GPU (slab k's GH prefix starts at its own first column; the walk is handed right to
    left), with stored words and with the recompute walk on each slab."""
    from globalign_amd import distributed
    if rc:
        set_knob(monkeypatch, "GA_RC", 1)
    case = gc.SLABS
    tables, s1, s2 = _tables(case)
    cost_ref, strings_ref, status_ref, mt_ref = _ref_chain(case, 21)[0]
    engines = [distributed.GpuSlabEngine(0) for _ in range(3)]
    try:
        cost, strings, status, mt_after = distributed.align_devices([0, 0, 0], s1, s2, tables.codes(s1), tables.codes(s2),
                                                                    tables, _mt(21), engines=engines)
    finally:
        for e in engines:
            e.eng.close()
    assert status == 0 and status_ref == "ok"
    assert int(cost) == cost_ref and tuple(strings) == strings_ref
    assert tuple(np.asarray(mt_after, dtype=np.uint32).tolist()) == mt_ref


# ---------------------------------------------------------------- public API (family S, a .mtx file)
@pytest.fixture()
def api(tmp_path):
    """-> (globalign_amd, settings with the family-S matrix file, scoring dict, costing dict)"""
    import globalign_amd
    tseed = gc.S1[1]
    letters, rows = gc.api_score_rows(tseed)
    path = gc.write_mtx(tmp_path / "general.mtx", letters, rows)
    smat, cmat = gc.api_tables(tseed)
    return globalign_amd, dict(scoring_mat_path=path, gap_open_score=-gc.BATCH_OPEN["S"]), smat, cmat


def _api_score(smat, cost, s1, s2):
    from oracle import transform
    return transform.cost_to_score(cost, len(s1), len(s2), transform.max_val(smat))


def _check_result(r, ref, smat, cmat, s1, s2):
    cost_ref, strings_ref, status_ref, _ = ref
    assert status_ref == "ok"
    assert r.cost == cost_ref and r.score == _api_score(smat, cost_ref, s1, s2)
    assert (r.seq_1_aligned, r.middle_part, r.seq_2_aligned) == strings_ref
    assert r.costing_mat == cmat and list(r.costing_mat.keys()) == list(cmat.keys())


@pytest.mark.parametrize("case", gc.API, ids=_ids(gc.API))
def test_api_find_global_alignment(api, case):
    ga, kw, smat, cmat = api
    _, s1, s2, o = _problem(case)
    ref = _ref_chain(case, 3)[0]
    random.seed(3)
    r = ga.find_global_alignment(seq_1=s1, seq_2=s2, **kw)
    _check_result(r, ref, smat, cmat, s1, s2)
    assert r.gap_open_cost == o
    assert random.getstate()[1] == ref[3]


def test_api_align_repeated(api):
    ga, kw, smat, cmat = api
    case = gc.API[1]
    _, s1, s2, _ = _problem(case)
    ref = _ref_chain(case, 4, 3)
    random.seed(4)
    runs = ga.GlobalAligner(**kw).align_repeated(s1, s2, 3)
    assert len(runs) == 3
    for r, one in zip(runs, ref):
        _check_result(r, one, smat, cmat, s1, s2)
    assert random.getstate()[1] == ref[-1][3]


def test_api_devices(api):
    ga, kw, smat, cmat = api
    case = gc.API[0]
    _, s1, s2, _ = _problem(case)
    ref = _ref_chain(case, 5)[0]
    random.seed(5)
    r = ga.GlobalAligner(devices=[0, 0], **kw).align(s1, s2)
    _check_result(r, ref, smat, cmat, s1, s2)
    assert random.getstate()[1] == ref[3]


def test_api_score_pairs_and_align_pairs(api):
    """20 edge pairs through score_pairs and align_pairs (seeds from a base past 2^32): costs, scores, strings."""
    from oracle import core
    ga, kw, smat, cmat = api
    cases = gc.batch_cases(gc.BATCH_API_SHAPES, gc.S1)
    assert len(cases) == 20
    pairs = [_problem(c)[1:3] for c in cases]
    want = np.array([_oracle_cost(c) for c in cases], dtype=np.int64)
    scores = np.array([_api_score(smat, int(c), s1, s2) for c, (s1, s2) in zip(want, pairs)], dtype=np.int64)
    al = ga.GlobalAligner(**kw)
    res = al.score_pairs([p[0] for p in pairs], [p[1] for p in pairs])
    assert np.array_equal(res.costs, want) and np.array_equal(res.scores, scores)
    base = 2 ** 32 - 7
    before = random.getstate()
    aligned = al.align_pairs([p[0] for p in pairs], [p[1] for p in pairs], seeds=base)
    assert random.getstate() == before
    assert np.array_equal(aligned.costs, want) and np.array_equal(aligned.scores, scores)
    for k, (case, (s1, s2)) in enumerate(zip(cases, pairs)):
        r = core.align(s1, s2, cmat, case[4], _mt(base + k))
        assert r["status"] == "ok"
        assert (aligned.seq_1_aligned[k], aligned.middle_part[k], aligned.seq_2_aligned[k]) == tuple(r["strings"]), case


def test_api_score_matrix(api):
    """5 x 4 sequences of edge lengths: the matrix is not symmetric under these tables, [i][j] is seqs[i] on the rows."""
    ga, kw, smat, cmat = api
    o = gc.BATCH_OPEN["S"]
    rows = [gc.splitmix_seq(L, 600 + L) for L in (2, 63, 65, 257, 513)]
    cols = [gc.splitmix_seq(L, 700 + L) for L in (3, 64, 129, 300)]
    res = ga.GlobalAligner(**kw).score_matrix(rows, cols)
    want = np.array([[gc.oracle_cost(cmat, x, y, o) for y in cols] for x in rows], dtype=np.int64)
    scores = np.array([[_api_score(smat, int(want[i][j]), x, y) for j, y in enumerate(cols)] for i, x in enumerate(rows)])
    assert res.costs.shape == (5, 4)
    assert np.array_equal(res.costs, want) and np.array_equal(res.scores, scores)
