"""Pipelined repeated alignments (ga_problem_align_many, GlobalAligner.align_repeated) vs the oracle.

`count` alignments of one pair must equal `count` consecutive find_global_alignment calls: alignment k
starts from the random state alignment k-1 left, so each k has its own tie-breaks.  The oracle runs the
same chain (core.align with the previous call's final state); strings, costs and every intermediate and
final random state must agree."""
import json
import os
import random

import numpy as np
import pytest

from tests.conftest import GOLDEN, aln_digest, load_matrix, splitmix_seq, state_digest, set_knob

pytestmark = pytest.mark.gpu


def _chain_oracle(s1, s2, kw, seed, count):
    from oracle import core, transform
    blosum = load_matrix(kw["scoring_mat_name"]) if kw.get("scoring_mat_name") else None
    a1, a2, _, cmat, _, goc = transform.settings(dict(kw, seq_1=s1, seq_2=s2), blosum=blosum)
    random.seed(seed)
    mt = core.mt_state_array()
    out = []
    for _ in range(count):
        r = core.align(a1, a2, cmat, goc, mt)
        mt = np.asarray(r["mt_out"], dtype=np.uint32)
        out.append((r["cost"], tuple(r["strings"]), mt.copy()))
    return out


@pytest.mark.parametrize("m,n,seed,count,kw", [
    (3000, 2500, 7, 4, dict(match_score=2, mismatch_score=-3, gap_open_score=-5, gap_extension_score=-1)),
    (1500, 1700, 8, 3, dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)),
    (900, 1000, 9, 2, dict(mismatch_cost=5, gap_open_cost=9, gap_extension_cost=3)),
    (2000, 64, 10, 5, dict(match_score=2, mismatch_score=-3, gap_open_score=-5, gap_extension_score=-1)),
])
def test_align_repeated_matches_chained_oracle(m, n, seed, count, kw):
    import globalign_amd
    alpha = "protein" if "scoring_mat_name" in kw else "dna"
    s1, s2 = splitmix_seq(m, seed, alpha), splitmix_seq(n, seed + 1, alpha)
    ref = _chain_oracle(s1, s2, kw, seed, count)
    random.seed(seed)
    runs = globalign_amd.GlobalAligner(max_seq_len_prod=None, **kw).align_repeated(s1, s2, count)
    assert len(runs) == count
    for r, (cost, strings, _) in zip(runs, ref):
        assert r.cost == cost
        assert (r.seq_1_aligned, r.middle_part, r.seq_2_aligned) == strings
    assert random.getstate()[1] == tuple(int(x) for x in ref[-1][2])
    # the same as `count` separate calls
    random.seed(seed)
    for cost, strings, _ in ref:
        r = globalign_amd.GlobalAligner(max_seq_len_prod=None, **kw).align(s1, s2)
        assert (r.seq_1_aligned, r.middle_part, r.seq_2_aligned) == strings
    assert random.getstate()[1] == tuple(int(x) for x in ref[-1][2])


def test_align_many_c3_first_matches_pin():
    """C3 size, three pipelined alignments: the first equals the oracle pin (tests/golden/c3_aln.json), all three
    reproduce both inputs at the golden cost, and each later one starts from the state the previous left."""
    import bench
    from globalign_amd import _native
    wl = bench.WORKLOADS["c3"]
    s1, s2 = bench.workload_pair(wl)
    tables, _ = bench.problem_tables(s1, s2, wl["scoring"])
    pin = json.load(open(os.path.join(GOLDEN, "c3_aln.json")))
    eng = _native.Engine(0)
    try:
        eng.load(tables.codes(s1), tables.codes(s2), tables)
        random.seed(0)
        mt0 = np.array(random.getstate()[1], dtype=np.uint32)
        runs, mt3 = eng.align_many(mt0, s1, s2, 3)
        cost0, (a, mid, b), st0 = runs[0]
        assert st0 == 0 and cost0 == pin["cost"] and len(mid) == pin["aln_len"]
        assert aln_digest(a, mid, b) == pin["aln_sha16"]
        for cost, (a, mid, b), st in runs:
            assert st == 0 and cost == pin["cost"]
            assert a.replace("-", "") == s1 and b.replace("-", "") == s2
        # alignment 1 = a single align() from the state alignment 0 left
        _, _, _, mt1 = eng.align(mt0, s1, s2)
        c1, strings1, _, mt2 = eng.align(mt1, s1, s2)
        assert strings1 == runs[1][1]
        _, strings2, _, mt3b = eng.align(mt2, s1, s2)
        assert strings2 == runs[2][1] and mt3.tolist() == mt3b.tolist()
    finally:
        eng.close()


@pytest.mark.parametrize("mode,fills", [("lane", "4"), ("lane", "3"), ("lane", "2"), ("row", "2"), ("row", "4")])
@pytest.mark.parametrize("m,n,seed,count,kw", [
    (2500, 3100, 11, 4, dict(match_score=2, mismatch_score=-3, gap_open_score=-5, gap_extension_score=-1)),
    (1200, 1300, 12, 3, dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)),
])
def test_align_repeated_pipe_modes(monkeypatch, mode, fills, m, n, seed, count, kw):
    """The pipeline's fill kernels (GA_PIPE_MODE: lane-skewed narrow fills / row-scan fills) and fills in
    flight give the chained oracle's strings, costs and final random state."""
    import globalign_amd
    set_knob(monkeypatch, "GA_PIPE_MODE", mode)
    set_knob(monkeypatch, "GA_PIPE_FILLS", fills)
    alpha = "protein" if "scoring_mat_name" in kw else "dna"
    s1, s2 = splitmix_seq(m, seed, alpha), splitmix_seq(n, seed + 1, alpha)
    ref = _chain_oracle(s1, s2, kw, seed, count)
    random.seed(seed)
    runs = globalign_amd.GlobalAligner(max_seq_len_prod=None, **kw).align_repeated(s1, s2, count)
    for r, (cost, strings, _) in zip(runs, ref):
        assert r.cost == cost
        assert (r.seq_1_aligned, r.middle_part, r.seq_2_aligned) == strings
    assert random.getstate()[1] == tuple(int(x) for x in ref[-1][2])


_CHAIN_SHAPES = [
    (700, 650, 13, 11, dict(match_score=2, mismatch_score=-3, gap_open_score=-5, gap_extension_score=-1)),
    (600, 640, 14, 9, dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)),
    (40000, 300, 15, 7, dict(match_score=2, mismatch_score=-3, gap_open_score=-5, gap_extension_score=-1)),
]
# every shape with and without the chain, and the smallest once more with the per-launch walks' result words and
# levels in device memory (GA_PIPE_PINNED_IO=0: read back with plain copies)
_CHAIN_CASES = [pytest.param(*s, chain, None, id=f"{s[0]}-{s[1]}-{s[2]}-{s[3]}-kw{q}-{chain}")
                for chain in ("1", "0") for q, s in enumerate(_CHAIN_SHAPES)]
_CHAIN_CASES.append(pytest.param(*_CHAIN_SHAPES[1], "0", "0", id="600-640-14-9-kw1-0-devio"))


@pytest.mark.parametrize("m,n,seed,count,kw,chain,pinned_io", _CHAIN_CASES)
def test_align_repeated_walk_chain(monkeypatch, chain, pinned_io, m, n, seed, count, kw):
    """Walks chained in one launch (walk_chain_kernel, opt-in GA_PIPE_CHAIN=1) and one launch per walk (the default):
    more alignments than slots (every slot reused), short walks that outrun the tie-break producer, a tall
    pair; each alignment's strings and cost and the final random state equal the chained oracle's."""
    import globalign_amd
    set_knob(monkeypatch, "GA_PIPE_CHAIN", chain)
    if pinned_io is not None:
        set_knob(monkeypatch, "GA_PIPE_PINNED_IO", pinned_io)
    alpha = "protein" if "scoring_mat_name" in kw else "dna"
    s1, s2 = splitmix_seq(m, seed, alpha), splitmix_seq(n, seed + 1, alpha)
    ref = _chain_oracle(s1, s2, kw, seed, count)
    random.seed(seed)
    runs = globalign_amd.GlobalAligner(max_seq_len_prod=None, **kw).align_repeated(s1, s2, count)
    for r, (cost, strings, _) in zip(runs, ref):
        assert r.cost == cost
        assert (r.seq_1_aligned, r.middle_part, r.seq_2_aligned) == strings
    assert random.getstate()[1] == tuple(int(x) for x in ref[-1][2])


def _assert_chained_oracle(m, n, seed, count, kw):
    import globalign_amd
    alpha = "protein" if "scoring_mat_name" in kw else "dna"
    s1, s2 = splitmix_seq(m, seed, alpha), splitmix_seq(n, seed + 1, alpha)
    ref = _chain_oracle(s1, s2, kw, seed, count)
    random.seed(seed)
    runs = globalign_amd.GlobalAligner(max_seq_len_prod=None, **kw).align_repeated(s1, s2, count)
    assert len(runs) == count
    for r, (cost, strings, _) in zip(runs, ref):
        assert r.cost == cost
        assert (r.seq_1_aligned, r.middle_part, r.seq_2_aligned) == strings
    assert random.getstate()[1] == tuple(int(x) for x in ref[-1][2])


@pytest.mark.parametrize("knobs,shape", [
    (dict(GA_PIPE_SLOTS=6), 0),
    (dict(GA_PIPE_SLOT_ORDER="fixed"), 0),
    (dict(GA_PIPE_FILL_PRIO="normal"), 1),
    (dict(GA_PIPE_CHAIN=1, GA_PIPE_SLOTS=6), 0),
], ids=["slots6", "fixed-order", "fill-prio-normal", "chain-slots6"])
def test_align_repeated_pipe_knobs(monkeypatch, knobs, shape):
    """The pipeline's other knobs: six slots (more than fills + 1) with per-launch walks and with the chain (which has
    six), walks that take slot k % S, fills on default-priority streams; more alignments than slots, so every slot is
    reused.  Strings, costs and the final random state equal the chained oracle's."""
    for k, v in knobs.items():
        set_knob(monkeypatch, k, v)
    _assert_chained_oracle(*_CHAIN_SHAPES[shape])


@pytest.mark.parametrize("m,n,seed,count,band_rows", [(900, 1000, 16, 1, None), (2500, 3100, 17, 3, 512)],
                         ids=["count1", "banded"])
def test_align_repeated_serial_fallback(monkeypatch, m, n, seed, count, band_rows):
    """One alignment, and banded tracebacks (GA_TB_BAND_ROWS: the band fills hold every CU): ga_problem_align_many
    runs them one after another, with the chained oracle's results."""
    if band_rows is not None:
        set_knob(monkeypatch, "GA_TB_BAND_ROWS", band_rows)
    _assert_chained_oracle(m, n, seed, count,
                           dict(match_score=2, mismatch_score=-3, gap_open_score=-5, gap_extension_score=-1))
