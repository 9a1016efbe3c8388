"""GlobalAligner.sample_alignments without a GPU: the samples / seeds validation and its order (seeds, then the
sequences, both before any engine exists), the flat seed numbering handed to the engine, BatchSamples.result and
.distinct, the empty call, and the host's share of ga_batch_sample -- the sample planner
(globalign_amd/csrc/ga_batch.h plan_batch_sample) and the walks' word address (ga_batch_layout.h) -- in a stand-alone
self-test, plain and under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "globalign_amd", "csrc")
LIB = os.path.join(ROOT, "globalign_amd", "_lib")


@pytest.fixture
def no_engine(monkeypatch):
    from globalign_amd import _native

    def refuse(*args, **kwargs):
        raise AssertionError("an engine was asked for before validation finished")

    monkeypatch.setattr(_native, "default_engine", refuse)
    monkeypatch.setattr(_native, "Engine", refuse)
    import globalign_amd
    return globalign_amd


A, B = ["ACGT", "AC"], ["ACGT", "AG"]


def test_exports():
    import globalign
    import globalign_amd
    assert "BatchSamples" in globalign_amd.__all__
    assert hasattr(globalign.GlobalAligner, "sample_alignments")


def test_unequal_lists(no_engine):
    with pytest.raises(ValueError):
        no_engine.GlobalAligner().sample_alignments(["ACGT", "AC"], ["ACGT"], samples=2)


def test_score_only_aligner_and_devices_are_refused(no_engine):
    with pytest.raises(ValueError) as e:
        no_engine.GlobalAligner(traceback=False).sample_alignments(["ACGT"], ["ACGT"], samples=2)
    assert "score_pairs" in str(e.value)
    with pytest.raises(ValueError):
        no_engine.GlobalAligner(devices=[0, 1]).sample_alignments(["ACGT"], ["ACGT"], samples=2)
    with pytest.raises(ValueError):
        no_engine.GlobalAligner().sample_alignments(["ACGT"], ["ACGT"], samples=2, tables="gpu")


@pytest.mark.parametrize("samples,seeds,error", [
    (None, 0, ValueError),                              # a base needs the counts
    (0, 0, ValueError), (-1, 0, ValueError),            # S >= 1
    ([1], 0, ValueError), ([1, 2, 3], 0, ValueError),   # one count per pair
    ([1, 0], 0, ValueError),
    (1.5, 0, TypeError), ([1, 2.0], 0, TypeError), ("2", 0, TypeError), ([1, "2"], 0, TypeError),
    (2, -1, ValueError), (2, 2 ** 64, ValueError),      # the base's range
    (2, 2 ** 64 - 3, ValueError),                       # base + 3 is too large
    (2, 1.5, TypeError), (2, "12", TypeError), (2, None, TypeError),
    (None, [[1, 2]], ValueError), (None, [[1], [2], [3]], ValueError),   # one list per pair
    (None, [[1], []], ValueError),                                       # at least one seed
    (None, [[1], [-1]], ValueError), (None, [[2 ** 64], [1]], ValueError),
    (None, [[1], [2.0]], TypeError), (None, [[1], ["2"]], TypeError), (None, [1, 2], TypeError),
    (None, [[1], "2"], TypeError), (None, [[1], None], TypeError),
    (2, [[1, 2], [3]], ValueError), ([2, 2], [[1, 2], [3]], ValueError),  # samples must agree
])
def test_bad_samples_and_seeds(no_engine, samples, seeds, error):
    with pytest.raises(error):
        no_engine.GlobalAligner().sample_alignments(A, B, samples=samples, seeds=seeds)


def test_seeds_are_checked_before_the_sequences(no_engine):
    with pytest.raises(ValueError) as e:
        no_engine.GlobalAligner().sample_alignments(["ACGT", "A-"], ["ACGT", ""], seeds=[[0], [-5]])
    assert "seed" in str(e.value)
    with pytest.raises(ValueError) as e:
        no_engine.GlobalAligner().sample_alignments(["ACGT", "A-"], ["ACGT", ""], samples=0, seeds=0)
    assert "samples" in str(e.value)


def test_sequence_validation_is_the_single_calls(no_engine):
    ga = no_engine

    def single_error(s1, s2, **kw):
        with pytest.raises(Exception) as e:
            ga.GlobalAligner(**kw).align(s1, s2)
        assert not isinstance(e.value, AssertionError)
        return e.value

    def same(got, want):
        assert type(got) is type(want) and str(got) == str(want)

    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner().sample_alignments(["ACGT", "AC-T", "A-"], ["ACGT", "ACGT", "ACGT"], samples=3, seeds=5)
    same(e.value, single_error("AC-T", "ACGT"))
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner().sample_alignments(["ACGT", "AC"], ["ACGT", ""], seeds=[[1, 2], [3]])
    same(e.value, single_error("AC", ""))
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner().sample_alignments(["ACGT"], ["ACЖT"], samples=2)
    assert "latin-1" in str(e.value)


def test_empty_call(no_engine):
    ga = no_engine
    state = random.getstate()
    for kw in (dict(), dict(samples=3), dict(samples=[]), dict(seeds=[]), dict(samples=3, seeds=2 ** 64 - 1)):
        res = ga.GlobalAligner().sample_alignments([], [], **kw)
        assert isinstance(res, ga.BatchSamples)
        assert res.seq_1_aligned == [] and res.middle_part == [] and res.seq_2_aligned == [] and res.seeds == []
        assert res.costs.shape == (0,) and res.scores.shape == (0,)
        assert res.costs.dtype == np.int64 and res.scores.dtype == np.int64
    res = ga.GlobalAligner(scoring_mat_name="BLOSUM62", gap_open_score=-10).sample_alignments([], [])
    assert res.gap_open_cost == 10 and res.gap_open_score == -10 and res.costing_mat["A"]["-"] == 10
    with pytest.raises(ValueError):
        ga.GlobalAligner().sample_alignments([], [], seeds=[[1]])
    with pytest.raises(ValueError):
        ga.GlobalAligner().sample_alignments([], [], samples=2, seeds=-1)
    assert random.getstate() == state


def _samples():
    import globalign_amd
    return globalign_amd.BatchSamples([["AC-T", "ACT-", "AC-T"], ["A"]], [["|| |", "||  ", "|| |"], ["*"]],
                                      [["ACGT", "ACGT", "ACGT"], ["C"]], np.array([3, 5]), np.array([4, -3]),
                                      [np.array([7, 8, 9], np.uint64), np.array([1], np.uint64)], {"A": {}}, {"C": {}},
                                      -4, 4)


def test_result_method():
    import globalign_amd
    res = _samples()
    r = res.result(0, 1)
    assert isinstance(r, globalign_amd.AlignmentResults)
    assert r == globalign_amd.AlignmentResults("ACT-", "||  ", "ACGT", 3, 4, {"A": {}}, {"C": {}}, -4, 4, None)
    assert type(r.cost) is int and type(r.score) is int
    assert res.result(1, 0)[:5] == ("A", "*", "C", 5, -3)
    with pytest.raises(IndexError):
        res.result(1, 1)


def test_distinct_method():
    res = _samples()
    assert res.distinct(0) == [(("AC-T", "|| |", "ACGT"), 2), (("ACT-", "||  ", "ACGT"), 1)]
    assert res.distinct(1) == [(("A", "*", "C"), 1)]


class _Recorder:
    """An engine that records what batch_sample is handed and answers with fixed buffers for 2 + 1 samples."""

    def __init__(self, seen, status=(0, 0, 0)):
        self.seen, self.status = seen, status

    def batch_sample(self, codes, seq_off, pair_a, pair_b, tables, sample_off, seeds, chars, pair_max_cost=None, **kw):
        self.seen.update(codes=codes, seq_off=seq_off, sample_off=sample_off, seeds=seeds, chars=bytes(chars),
                         pair_max_cost=pair_max_cost, kw=kw)
        bufs = tuple(np.frombuffer(t, dtype=np.uint8) for t in (b"AC-TxACT-yyAA", b"|| |x||  yy* ", b"ACGTxACGTyyC-"))
        return (np.arange(len(pair_a), dtype=np.int64), np.array(self.status, dtype=np.int32),
                np.array([4, 4, 2], dtype=np.int64), np.array([0, 5, 11, 13], dtype=np.int64), bufs)


def test_engine_gets_flat_seeds_characters_and_own_max_cost(monkeypatch):
    """With a base the samples are numbered flat in pair order and sample f gets base + f; with nested seeds the
    engine gets them concatenated.  The strings are cut from its buffers at its offsets, per pair and sample."""
    import globalign_amd
    from globalign_amd import _native
    seen = {}
    monkeypatch.setattr(_native, "default_engine", lambda device=0: _Recorder(seen))
    kw = dict(match_score=1, mismatch_score=-5, gap_open_score=-60, gap_extension_score=-1)
    state = random.getstate()
    res = globalign_amd.GlobalAligner(**kw).sample_alignments(["acgt", "AA"], ["ACGT", "A"], samples=[2, 1],
                                                              seeds=2 ** 64 - 3)
    assert random.getstate() == state
    assert seen["seeds"].dtype == np.uint64 and seen["seeds"].tolist() == [2 ** 64 - 3, 2 ** 64 - 2, 2 ** 64 - 1]
    assert seen["sample_off"].dtype == np.int64 and seen["sample_off"].tolist() == [0, 2, 3]
    assert seen["chars"] == b"ACGTAAACGTA" and len(seen["codes"]) == 11 and seen["seq_off"].tolist() == [0, 4, 6, 10, 11]
    assert seen["pair_max_cost"].tolist() == [6, 2] and seen["kw"] == {}
    assert isinstance(res, globalign_amd.BatchSamples)
    assert res.seq_1_aligned == [["AC-T", "ACT-"], ["AA"]] and res.middle_part == [["|| |", "||  "], ["* "]]
    assert res.seq_2_aligned == [["ACGT", "ACGT"], ["C-"]]
    assert res.costs.tolist() == [0, 1] and res.scores.tolist() == [4, 1]
    assert [s.tolist() for s in res.seeds] == [[2 ** 64 - 3, 2 ** 64 - 2], [2 ** 64 - 1]]
    assert all(s.dtype == np.uint64 for s in res.seeds)
    res = globalign_amd.GlobalAligner(**kw).sample_alignments(["acgt", "AA"], ["ACGT", "A"], seeds=[[7, 7], [2 ** 63]],
                                                              tables="device")
    assert seen["seeds"].tolist() == [7, 7, 2 ** 63] and seen["sample_off"].tolist() == [0, 2, 3]
    assert seen["kw"] == {"rng_tables": "device"}
    assert [s.tolist() for s in res.seeds] == [[7, 7], [2 ** 63]]


def test_an_int_gives_every_pair_that_many_samples(monkeypatch):
    import globalign_amd
    from globalign_amd import _native
    seen = {}

    class Uniform:
        def batch_sample(self, codes, seq_off, pair_a, pair_b, tables, sample_off, seeds, chars, pair_max_cost=None):
            seen.update(sample_off=sample_off, seeds=seeds)
            S = len(seeds)
            bufs = tuple(np.frombuffer(t * S, dtype=np.uint8) for t in (b"Ax", b"|x", b"Ax"))
            return (np.zeros(len(pair_a), dtype=np.int64), np.zeros(S, dtype=np.int32), np.ones(S, dtype=np.int64),
                    2 * np.arange(S + 1, dtype=np.int64), bufs)

    monkeypatch.setattr(_native, "default_engine", lambda device=0: Uniform())
    res = globalign_amd.GlobalAligner().sample_alignments(["A", "AA", "AAA"], ["A", "A", "A"], samples=2, seeds=10)
    assert seen["seeds"].tolist() == [10, 11, 12, 13, 14, 15] and seen["sample_off"].tolist() == [0, 2, 4, 6]
    assert res.seq_1_aligned == [["A", "A"]] * 3 and res.middle_part == [["|", "|"]] * 3
    assert [s.tolist() for s in res.seeds] == [[10, 11], [12, 13], [14, 15]]
    assert res.distinct(2) == [(("A", "|", "A"), 2)]


def test_index_error_names_the_lowest_pair(monkeypatch):
    import globalign_amd
    from globalign_amd import _native
    monkeypatch.setattr(_native, "default_engine", lambda device=0: _Recorder({}, status=(0, 0, 1)))
    with pytest.raises(IndexError) as e:
        globalign_amd.GlobalAligner().sample_alignments(["AC", "A"], ["AC", "ACGT"], samples=[2, 1])
    assert str(e.value) == "pair 1: string index out of range"
    monkeypatch.setattr(_native, "default_engine", lambda device=0: _Recorder({}, status=(0, 1, 1)))
    with pytest.raises(IndexError) as e:
        globalign_amd.GlobalAligner().sample_alignments(["AC", "A"], ["AC", "ACGT"], samples=[2, 1])
    assert str(e.value) == "pair 0: string index out of range"


def test_native_exports_the_new_entries():
    from globalign_amd import _native
    lib = _native.load_library()
    for name in ("ga_batch_sample", "ga_batch_sample_info", "ga_batch_sample_timings"):
        assert name in _native.EXPORTS and hasattr(lib, name)


# ---------------------------------------------------------------- the host self-test
@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-s", "-C", CSRC, "batch_sample_selftest", "batch_sample_asan"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return True


@pytest.mark.parametrize("binary", ["ga_batch_sample_selftest_asan", "ga_batch_sample_selftest"])
def test_host_selftest(built, binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(LIB, binary)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
