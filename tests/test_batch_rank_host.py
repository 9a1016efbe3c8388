"""GlobalAligner.alignments_by_rank, enumerate_alignments and sample_alignments_uniform without a GPU: the exports, the
validation and its order (count_alignments's, then the ranks, then the two-letter rule, all before any engine exists),
the empty call, what the engine is handed by all three methods, BatchRanked.complete, the host's share of ga_batch_rank
-- the CPU model of the saturating count table and of the unranking walk, the table's address function
(globalign_amd/csrc/ga_batch_rank.h) and the rank planner (ga_batch.h plan_batch_rank) -- in a stand-alone self-test,
plain and under AddressSanitizer + UndefinedBehaviorSanitizer, and the pure-Python expected alignments
(tests/alignment_ranks.py) pinned against the reference's own traceback."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import alignment_counts as ac
from tests import alignment_ranks as ar
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "globalign_amd", "csrc")
LIB = os.path.join(ROOT, "globalign_amd", "_lib")
CAP = 2 ** 64 - 1
FIELDS = ("seq_1_aligned", "middle_part", "seq_2_aligned", "costs", "scores", "ranks", "counts", "saturated",
          "scoring_mat", "costing_mat", "gap_open_score", "gap_open_cost")
METHODS = ("alignments_by_rank", "enumerate_alignments", "sample_alignments_uniform")


@pytest.fixture
def no_engine(monkeypatch):
    from globalign_amd import _native

    def refuse(*args, **kwargs):
        raise AssertionError("an engine was asked for before validation finished")

    monkeypatch.setattr(_native, "default_engine", refuse)
    monkeypatch.setattr(_native, "Engine", refuse)
    import globalign_amd
    return globalign_amd


def _call(al, method, seqs_1, seqs_2, ranks=None):
    """The method on the lists, with arguments that are valid whenever the lists are."""
    if method == "alignments_by_rank":
        return al.alignments_by_rank(seqs_1, seqs_2, [[0]] * len(list(seqs_1)) if ranks is None else ranks)
    if method == "enumerate_alignments":
        return al.enumerate_alignments(seqs_1, seqs_2)
    return al.sample_alignments_uniform(seqs_1, seqs_2, 2, seed=1)


def test_exports():
    import globalign
    import globalign_amd
    assert "BatchRanked" in globalign_amd.__all__ and hasattr(globalign_amd, "BatchRanked")
    assert globalign_amd.BatchRanked._fields == FIELDS
    for name in METHODS:
        assert hasattr(globalign_amd.GlobalAligner, name) and hasattr(globalign.GlobalAligner, name)


def test_native_exports_the_new_entries():
    from globalign_amd import _native
    lib = _native.load_library()
    for name in ("ga_batch_rank", "ga_batch_rank_info", "ga_batch_rank_timings"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    for name in ("batch_rank", "batch_rank_info", "batch_rank_timings"):
        assert hasattr(_native.Engine, name)
    header = open(os.path.join(ROOT, "include", "globalign_amd.h")).read()
    for name in ("ga_batch_rank(", "ga_batch_rank_info(", "ga_batch_rank_timings(", "rank_off", "rank_status",
                 "GA_BATCH_RANK_TABLE_BYTES", "uint64_t* count_out"):
        assert name in header


@pytest.mark.parametrize("method", METHODS)
def test_list_and_aligner_validation_is_count_alignments(no_engine, method):
    ga = no_engine
    with pytest.raises(ValueError) as e:
        _call(ga.GlobalAligner(), method, ["ACGT", "AC"], ["ACGT"])
    assert f"{method} needs as many first as second sequences" in str(e.value)
    with pytest.raises(ValueError) as e:
        _call(ga.GlobalAligner(traceback=False), method, ["ACGT"], ["ACGT"])
    assert "score_pairs" in str(e.value)
    with pytest.raises(ValueError) as e:
        _call(ga.GlobalAligner(devices=[0, 1]), method, ["ACGT"], ["ACGT"])
    assert "one GPU" in str(e.value)
    # the order: the lists, then traceback, then the devices
    with pytest.raises(ValueError) as e:
        _call(ga.GlobalAligner(traceback=False, devices=[0, 1]), method, ["ACGT"], [])
    assert "as many first as second" in str(e.value)
    with pytest.raises(ValueError) as e:
        _call(ga.GlobalAligner(traceback=False, devices=[0, 1]), method, ["ACGT"], ["ACGT"])
    assert "score_pairs" in str(e.value)


@pytest.mark.parametrize("method", METHODS)
def test_sequence_validation_is_the_single_calls(no_engine, method):
    ga = no_engine

    def single_error(s1, s2, **kw):
        with pytest.raises(Exception) as e:
            ga.GlobalAligner(**kw).align(s1, s2)
        assert not isinstance(e.value, AssertionError)
        return e.value

    def same(got, want):
        assert type(got) is type(want) and str(got) == str(want)

    with pytest.raises(RuntimeError) as e:
        _call(ga.GlobalAligner(), method, ["ACGT", "AC-T", "A-"], ["ACGT", "ACGT", "ACGT"])
    same(e.value, single_error("AC-T", "ACGT"))
    with pytest.raises(RuntimeError) as e:
        _call(ga.GlobalAligner(), method, ["ACGT", "AC"], ["ACGT", ""])
    same(e.value, single_error("AC", ""))
    with pytest.raises(ValueError) as e:
        _call(ga.GlobalAligner(), method, ["ACGT"], ["ACЖT"])
    assert "latin-1" in str(e.value)
    with pytest.raises(TypeError):
        _call(ga.GlobalAligner(), method, ["ACGT"], [5])
    # the sequences' own faults come before the two-letter rule
    with pytest.raises(RuntimeError) as e:
        _call(ga.GlobalAligner(), method, ["A", "AC-T"], ["ACGT", "ACGT"])
    same(e.value, single_error("AC-T", "ACGT"))


def test_ranks_validation(no_engine):
    al = no_engine.GlobalAligner()
    two = (["ACGT", "AC"], ["ACGT", "CA"])
    with pytest.raises(ValueError) as e:
        al.alignments_by_rank(*two, [[0]])
    assert str(e.value) == "ranks must have one entry per pair, got 1 for 2 pairs"
    for bad in (5, "01", [0, 1], [[0], 1], [[0], "1"]):
        with pytest.raises(TypeError):
            al.alignments_by_rank(*two, bad)
    for bad in ([[0], [1.0]], [[0], ["1"]], [[None], []]):
        with pytest.raises(TypeError) as e:
            al.alignments_by_rank(*two, bad)
        assert "ranks must be ints" in str(e.value)
    for bad in ([[0], [-1]], [[CAP], []], [[0, 2 ** 70], [0]]):
        with pytest.raises(ValueError) as e:
            al.alignments_by_rank(*two, bad)
        assert "every rank must be in [0, 2**64 - 1)" in str(e.value)
    # the sequences' faults come first, the ranks' before the two-letter rule
    with pytest.raises(RuntimeError):
        al.alignments_by_rank(["AC-T"], ["ACGT"], [])
    with pytest.raises(ValueError) as e:
        al.alignments_by_rank(["A"], ["ACGT"], [])
    assert "one entry per pair" in str(e.value)
    with pytest.raises(TypeError):
        al.alignments_by_rank(["A"], ["ACGT"], [[0.5]])
    # enumerate_alignments's limit and sample_alignments_uniform's samples and seed
    for bad in (0, -3):
        with pytest.raises(ValueError) as e:
            al.enumerate_alignments(*two, limit=bad)
        assert str(e.value) == "limit must be at least 1"
    with pytest.raises(TypeError):
        al.enumerate_alignments(*two, limit=2.5)
    with pytest.raises(ValueError):
        al.sample_alignments_uniform(*two, 0)
    with pytest.raises(ValueError):
        al.sample_alignments_uniform(*two, [1])
    with pytest.raises(TypeError):
        al.sample_alignments_uniform(*two, [1, 2.0])
    with pytest.raises(TypeError):
        al.sample_alignments_uniform(*two, 2, seed="7")


@pytest.mark.parametrize("method", METHODS)
def test_one_letter_sequences_are_refused_for_the_lowest_pair(no_engine, method):
    ga = no_engine
    with pytest.raises(ValueError) as e:
        _call(ga.GlobalAligner(), method, ["ACGT", "ACG", "A", "C"], ["ACGT", "T", "ACGT", "G"])
    assert str(e.value) == f"pair 1: {method} needs sequences of at least two letters"
    with pytest.raises(ValueError) as e:
        _call(ga.GlobalAligner(scoring_mat_name="BLOSUM62"), method, ["W"], ["WW"])
    assert str(e.value) == f"pair 0: {method} needs sequences of at least two letters"


@pytest.mark.parametrize("method", METHODS)
def test_empty_call(no_engine, method):
    ga = no_engine
    state = random.getstate()
    res = _call(ga.GlobalAligner(), method, [], [])
    assert isinstance(res, ga.BatchRanked)
    assert res.seq_1_aligned == [] and res.middle_part == [] and res.seq_2_aligned == [] and res.ranks == []
    assert res.counts.shape == (0,) and res.counts.dtype == np.uint64
    assert res.saturated.shape == (0,) and res.saturated.dtype == np.bool_
    assert res.costs.shape == (0,) and res.scores.shape == (0,)
    assert res.costs.dtype == np.int64 and res.scores.dtype == np.int64
    assert res.scoring_mat is None and res.gap_open_cost == 4
    res = _call(ga.GlobalAligner(scoring_mat_name="BLOSUM62", gap_open_score=-10), method, iter([]), ())
    assert res.gap_open_cost == 10 and res.gap_open_score == -10 and res.costing_mat["A"]["-"] == 10
    with pytest.raises(ValueError):
        _call(ga.GlobalAligner(traceback=False), method, [], [])
    assert random.getstate() == state


def test_complete():
    import globalign_amd

    def res(ranks, counts):
        counts = np.array(counts, dtype=np.uint64)
        return globalign_amd.BatchRanked([[""] * len(r) for r in ranks], [[""] * len(r) for r in ranks],
                                         [[""] * len(r) for r in ranks], np.zeros(len(ranks), dtype=np.int64),
                                         np.zeros(len(ranks), dtype=np.int64),
                                         [np.array(r, dtype=np.uint64) for r in ranks], counts, counts == np.uint64(CAP),
                                         {}, {}, -4, 4)

    r = res([[0, 1, 2], [0, 1], [0, 2, 1], [1, 2, 3], [], [0], [0, 0, 1], [0, 1, 2]], [3, 3, 3, 3, 1, 1, 3, CAP])
    assert [r.complete(k) for k in range(8)] == [True, False, False, False, False, True, False, False]
    assert r.saturated.tolist() == [False] * 7 + [True]
    with pytest.raises(IndexError):
        r.complete(8)
    one = r.result(0, 1)
    assert isinstance(one, globalign_amd.AlignmentResults) and one.cost == 0 and one.gap_open_cost == 4


class _Recorder:
    """An engine that records what batch_rank is handed and answers from fixed counts: every slot's three strings are
    'r<rank>', 'm<rank>' and 'b<rank>'."""

    def __init__(self, calls, counts):
        self.calls, self.counts = calls, counts

    def batch_rank(self, codes, seq_off, pair_a, pair_b, tables, rank_off, ranks, chars, pair_max_cost=None, **kw):
        self.calls.append(dict(codes=codes, seq_off=seq_off, pair_a=pair_a, pair_b=pair_b, tables=tables,
                               rank_off=np.array(rank_off), ranks=np.array(ranks), chars=chars,
                               pair_max_cost=pair_max_cost, kw=kw))
        counts = np.array(self.counts, dtype=np.uint64)
        status = np.array([int(r) >= self.counts[int(np.searchsorted(rank_off, f, side="right")) - 1]
                           for f, r in enumerate(ranks)], dtype=np.int32)
        texts = [[pre + str(int(r)) for r in ranks] for pre in ("r", "m", "b")]
        lengths = np.array([len(t) for t in texts[1]], dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(lengths + 1)]).astype(np.int64)
        bufs = []
        for line in texts:
            buf = np.zeros(max(int(offsets[-1]), 1), dtype=np.uint8)
            for f, t in enumerate(line):
                buf[offsets[f]:offsets[f] + len(t)] = np.frombuffer(t.encode(), dtype=np.uint8)
            bufs.append(buf)
        return np.arange(len(pair_a), dtype=np.int64), counts, status, lengths, offsets, tuple(bufs)


KW = dict(match_score=1, mismatch_score=-5, gap_open_score=-60, gap_extension_score=-1)
SEQS = (["acgt", "AA", "GGT"], ["ACGT", "AA", "TG"])


def _recorded(monkeypatch, counts):
    import globalign_amd
    from globalign_amd import _native
    calls = []
    monkeypatch.setattr(_native, "default_engine", lambda device=0: _Recorder(calls, counts))
    return globalign_amd, calls


def test_alignments_by_rank_hands_the_engine_the_batch_and_the_ranks(monkeypatch):
    ga, calls = _recorded(monkeypatch, [30, CAP, 5])
    state = random.getstate()
    res = ga.GlobalAligner(**KW).alignments_by_rank(*SEQS, [[7, 0, 29], (), np.array([4, 4])])
    assert random.getstate() == state
    assert len(calls) == 1
    seen = calls[0]
    assert len(seen["codes"]) == 17 and seen["codes"].dtype == np.uint8
    assert seen["seq_off"].tolist() == [0, 4, 6, 9, 13, 15, 17]
    assert seen["pair_a"].tolist() == [0, 1, 2] and seen["pair_b"].tolist() == [3, 4, 5]
    assert seen["pair_max_cost"].tolist() == [6, 2, 6] and seen["kw"] == {}
    assert seen["tables"].gap_open == 60
    assert seen["rank_off"].tolist() == [0, 3, 3, 5] and seen["rank_off"].dtype == np.int64
    assert seen["ranks"].tolist() == [7, 0, 29, 4, 4] and seen["ranks"].dtype == np.uint64
    assert bytes(seen["chars"]) == b"ACGTAAGGTACGTAATG"
    assert isinstance(res, ga.BatchRanked)
    assert res.seq_1_aligned == [["r7", "r0", "r29"], [], ["r4", "r4"]]
    assert res.middle_part == [["m7", "m0", "m29"], [], ["m4", "m4"]]
    assert res.seq_2_aligned == [["b7", "b0", "b29"], [], ["b4", "b4"]]
    assert [r.tolist() for r in res.ranks] == [[7, 0, 29], [], [4, 4]] and all(r.dtype == np.uint64 for r in res.ranks)
    assert res.counts.dtype == np.uint64 and res.counts.tolist() == [30, CAP, 5]
    assert res.saturated.dtype == np.bool_ and res.saturated.tolist() == [False, True, False]
    assert res.costs.tolist() == [0, 1, 2] and res.scores.tolist() == [4, 1, 1]
    assert res.gap_open_cost == 60 and res.gap_open_score == -60 and res.costing_mat["A"]["C"] == 6
    assert res.result(2, 1).seq_2_aligned == "b4" and res.result(0, 0).cost == 0
    assert not res.complete(0) and not res.complete(1)
    # a rank that is not below its pair's count: the lowest pair and slot
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner(**KW).alignments_by_rank(*SEQS, [[3], [CAP - 1], [2, 5, 9]])
    assert str(e.value) == "pair 2: rank 5 is not below the pair's count 5"
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner(**KW).alignments_by_rank(*SEQS, [[30, 31], [], [7]])
    assert str(e.value) == "pair 0: rank 30 is not below the pair's count 30"


def test_enumerate_alignments_counts_then_asks_for_the_first_ranks(monkeypatch):
    ga, calls = _recorded(monkeypatch, [3, CAP, 2000])
    state = random.getstate()
    res = ga.GlobalAligner(**KW).enumerate_alignments(*SEQS, limit=5)
    assert random.getstate() == state
    assert len(calls) == 2
    assert calls[0]["rank_off"].tolist() == [0, 0, 0, 0] and calls[0]["ranks"].tolist() == []
    assert calls[1]["rank_off"].tolist() == [0, 3, 8, 13]
    assert calls[1]["ranks"].tolist() == [0, 1, 2, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4]
    assert [res.complete(k) for k in range(3)] == [True, False, False]
    assert res.seq_1_aligned[0] == ["r0", "r1", "r2"]
    res = ga.GlobalAligner(**KW).enumerate_alignments(*SEQS)
    assert calls[3]["rank_off"].tolist() == [0, 3, 1027, 2051]      # the default limit is 1024
    assert not res.complete(2)
    res = ga.GlobalAligner(**KW).enumerate_alignments(*SEQS, limit=2000)
    assert res.complete(2) and not res.complete(1) and len(res.ranks[1]) == 2000


def test_sample_alignments_uniform_draws_the_documented_ranks(monkeypatch):
    counts = [3, 10 ** 15, 2000]
    ga, calls = _recorded(monkeypatch, counts)
    state = random.getstate()
    res = ga.GlobalAligner(**KW).sample_alignments_uniform(*SEQS, [4, 1, 3], seed=11)
    assert random.getstate() == state
    assert len(calls) == 2 and calls[0]["ranks"].tolist() == [] and calls[0]["rank_off"].tolist() == [0, 0, 0, 0]
    rng = random.Random(11)
    want = [[rng.randrange(counts[k]) for _ in range(s)] for k, s in enumerate([4, 1, 3])]
    assert calls[1]["rank_off"].tolist() == [0, 4, 5, 8]
    assert calls[1]["ranks"].tolist() == [r for own in want for r in own]
    assert [r.tolist() for r in res.ranks] == want
    # an int for every pair, the default seed, and reproducibility
    again = ga.GlobalAligner(**KW).sample_alignments_uniform(*SEQS, 2)
    rng = random.Random(0)
    assert [r.tolist() for r in again.ranks] == [[rng.randrange(c) for _ in range(2)] for c in counts]
    twice = ga.GlobalAligner(**KW).sample_alignments_uniform(*SEQS, 2)
    assert [r.tolist() for r in twice.ranks] == [r.tolist() for r in again.ranks]
    # a saturated pair cannot be indexed by a u64: the lowest such pair
    ga, calls = _recorded(monkeypatch, [3, CAP, CAP])
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner(**KW).sample_alignments_uniform(*SEQS, 2)
    assert str(e.value).startswith("pair 1: the count is saturated")
    assert len(calls) == 1


# ---------------------------------------------------------------- the expected-alignments helper against the reference
def _reference_set(s1, s2, cmat, o):
    seen = set()
    for s in ac.PINNED_SEEDS:
        words = np.array(random.Random(s).getstate()[1], dtype=np.uint32)
        got = ac.core.align(s1, s2, cmat, o, words)
        assert got["status"] == "ok"
        seen.add((got["strings"][0], got["strings"][1], got["strings"][2]))
    return seen


@pytest.mark.parametrize("s1,s2,count", ac.PINNED)
def test_helper_ranks_what_the_reference_returns(s1, s2, count):
    """Over ranks 0 .. count - 1 the helper gives exactly the alignments the reference's traceback returns over the
    pinned seed range -- all three lines --, in depth-first order of the traceback's levels."""
    cmat, o = ac.costs_of()
    R = ar.ranked(s1, s2, cmat, o)
    assert R.count == count == ac.expected_count(s1, s2, cmat, o)[0]
    got = [R.strings(r) for r in range(count)]
    ref = _reference_set(s1, s2, cmat, o)
    assert len(set(got)) == count and set(got) == ref
    assert {(a, b) for a, _, b in got} == {(a, b) for a, _, b in ref}
    levels = [R.levels(r) for r in range(count)]
    assert levels == R.all_levels() and levels == sorted(levels)
    dp = ac.filled_array(s1, s2, cmat, o)
    assert all(ar.alignment_cost(t, cmat, o) == dp[len(s1), len(s2)].min() for t in got)


def test_helper_on_a_fully_tied_table():
    sets = np.full((2, 2), 0x1ff, dtype=np.int64)
    R = ar.Ranked("AC", "GT", sets)
    assert R.count == 13 and len({tuple(x) for x in R.all_levels()}) == 13
    assert [R.levels(r) for r in range(13)] == R.all_levels()
    assert R.strings(0) == ("AC", "**", "GT") and R.strings(12) == ("--AC", "    ", "GT--")
    big = ar.Ranked("A" * 40, "C" * 40, np.full((40, 40), 0x1ff, dtype=np.int64))
    assert big.count == ac.count_from_sets(np.full((40, 40), 0x1ff, dtype=np.int64))[0] > CAP
    assert big.levels(0) == [0] * 40 and big.levels(big.count - 1)[:40] == [2] * 40


# ---------------------------------------------------------------- the host self-test
@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-s", "-C", CSRC, "batch_rank_selftest", "batch_rank_asan"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return True


@pytest.mark.parametrize("binary", ["ga_batch_rank_selftest_asan", "ga_batch_rank_selftest"])
def test_host_selftest(built, binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(LIB, binary)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_table_knob_is_an_option_and_not_an_environment_variable():
    opts = open(os.path.join(CSRC, "ga_opts.h")).read()
    assert '"GA_BATCH_RANK_TABLE_BYTES"' in opts
    env_knobs = opts[opts.index("kEnvKnobs[] = {"):opts.index("inline bool env_knob")]
    assert "GA_BATCH_RANK_TABLE_BYTES" not in env_knobs
