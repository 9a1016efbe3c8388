"""GlobalAligner.count_alignments without a GPU: the exports, the validation and its order (align_pairs's, then the
two-letter rule, all before any engine exists), the empty call, BatchCounts.count and .exact, what the engine is
handed, the host's share of ga_batch_count -- the count planner (globalign_amd/csrc/ga_batch.h plan_batch_count) and
the CPU model of the recurrence (ga_batch_count.h) -- in a stand-alone self-test, plain and under AddressSanitizer +
UndefinedBehaviorSanitizer, and the pure-Python expected count (tests/alignment_counts.py) pinned against the
reference's own traceback."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import alignment_counts as ac
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


def test_exports():
    import globalign
    import globalign_amd
    assert "BatchCounts" in globalign_amd.__all__
    assert hasattr(globalign_amd, "BatchCounts")
    assert hasattr(globalign.GlobalAligner, "count_alignments")
    assert globalign_amd.BatchCounts._fields == ("counts", "exact", "costs", "scores", "scoring_mat", "costing_mat",
                                                 "gap_open_score", "gap_open_cost")


def test_native_exports_the_new_entries():
    from globalign_amd import _native
    lib = _native.load_library()
    for name in ("ga_batch_count", "ga_batch_count_info", "ga_batch_count_timings"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "globalign_amd.h")).read()
    for name in ("ga_batch_count(", "ga_batch_count_info(", "ga_batch_count_timings("):
        assert name in header


def test_unequal_lists(no_engine):
    with pytest.raises(ValueError) as e:
        no_engine.GlobalAligner().count_alignments(["ACGT", "AC"], ["ACGT"])
    assert "count_alignments needs as many first as second sequences" in str(e.value)


def test_score_only_aligner_and_devices_are_refused(no_engine):
    with pytest.raises(ValueError) as e:
        no_engine.GlobalAligner(traceback=False).count_alignments(["ACGT"], ["ACGT"])
    assert "score_pairs" in str(e.value)
    with pytest.raises(ValueError) as e:
        no_engine.GlobalAligner(devices=[0, 1]).count_alignments(["ACGT"], ["ACGT"])
    assert "one GPU" in str(e.value)
    # the order is align_pairs's: the lists, then traceback, then the devices
    with pytest.raises(ValueError) as e:
        no_engine.GlobalAligner(traceback=False, devices=[0, 1]).count_alignments(["ACGT"], [])
    assert "as many first as second" in str(e.value)
    with pytest.raises(ValueError) as e:
        no_engine.GlobalAligner(traceback=False, devices=[0, 1]).count_alignments(["ACGT"], ["ACGT"])
    assert "score_pairs" in str(e.value)


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
        ga.GlobalAligner().count_alignments(["ACGT", "AC-T", "A-"], ["ACGT", "ACGT", "ACGT"])
    same(e.value, single_error("AC-T", "ACGT"))
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner().count_alignments(["ACGT", "AC"], ["ACGT", ""])
    same(e.value, single_error("AC", ""))
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner().count_alignments(["ACGT"], ["ACЖT"])
    assert "latin-1" in str(e.value)
    with pytest.raises(TypeError):
        ga.GlobalAligner().count_alignments(["ACGT"], [5])
    # the sequences' own faults come before the two-letter rule
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner().count_alignments(["A", "AC-T"], ["ACGT", "ACGT"])
    same(e.value, single_error("AC-T", "ACGT"))


def test_one_letter_sequences_are_refused_for_the_lowest_pair(no_engine):
    ga = no_engine
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner().count_alignments(["ACGT", "ACG", "A", "C"], ["ACGT", "T", "ACGT", "G"])
    assert str(e.value) == "pair 1: count_alignments needs sequences of at least two letters"
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner(scoring_mat_name="BLOSUM62").count_alignments(["W"], ["WW"])
    assert str(e.value) == "pair 0: count_alignments needs sequences of at least two letters"
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner().count_alignments(["AA", "a"], ["AA", "aa"])
    assert str(e.value) == "pair 1: count_alignments needs sequences of at least two letters"


def test_empty_call(no_engine):
    ga = no_engine
    state = random.getstate()
    res = ga.GlobalAligner().count_alignments([], [])
    assert isinstance(res, ga.BatchCounts)
    assert res.counts.shape == (0,) and res.counts.dtype == np.float64
    assert res.exact.shape == (0,) and res.exact.dtype == np.bool_
    assert res.costs.shape == (0,) and res.scores.shape == (0,)
    assert res.costs.dtype == np.int64 and res.scores.dtype == np.int64
    assert res.scoring_mat is None and res.gap_open_cost == 4
    res = ga.GlobalAligner(scoring_mat_name="BLOSUM62", gap_open_score=-10).count_alignments(iter([]), ())
    assert res.gap_open_cost == 10 and res.gap_open_score == -10 and res.costing_mat["A"]["-"] == 10
    with pytest.raises(ValueError):
        ga.GlobalAligner(traceback=False).count_alignments([], [])
    assert random.getstate() == state


def test_count_method_and_exact():
    import globalign_amd
    counts = np.array([1.0, 7.0, 2.0 ** 53 - 1, 2.0 ** 53, 1e300, np.inf])
    res = globalign_amd.BatchCounts(counts, counts < 2.0 ** 53, np.arange(6), -np.arange(6), {"A": {}}, {"C": {}}, -4, 4)
    assert res.exact.tolist() == [True, True, True, False, False, False]
    assert [type(res.count(k)) for k in range(6)] == [int, int, int, float, float, float]
    assert res.count(1) == 7 and res.count(2) == 2 ** 53 - 1 and res.count(3) == 2.0 ** 53 and res.count(5) == float("inf")
    assert res.count(-1) == float("inf")
    with pytest.raises(IndexError):
        res.count(6)


class _Recorder:
    """An engine that records what batch_count is handed and answers with fixed costs and counts."""

    def __init__(self, seen, counts):
        self.seen, self.counts = seen, counts

    def batch_count(self, codes, seq_off, pair_a, pair_b, tables, pair_max_cost=None, **kw):
        self.seen.update(codes=codes, seq_off=seq_off, pair_a=pair_a, pair_b=pair_b, tables=tables,
                         pair_max_cost=pair_max_cost, kw=kw)
        return np.arange(len(pair_a), dtype=np.int64), np.array(self.counts, dtype=np.float64)


def test_engine_gets_the_batch_and_its_own_max_cost(monkeypatch):
    import globalign_amd
    from globalign_amd import _native
    seen = {}
    monkeypatch.setattr(_native, "default_engine", lambda device=0: _Recorder(seen, [3.0, 2.0 ** 60, np.inf]))
    kw = dict(match_score=1, mismatch_score=-5, gap_open_score=-60, gap_extension_score=-1)
    state = random.getstate()
    res = globalign_amd.GlobalAligner(**kw).count_alignments(["acgt", "AA", "GGT"], ["ACGT", "AA", "TG"])
    assert random.getstate() == state
    assert len(seen["codes"]) == 17 and seen["codes"].dtype == np.uint8
    assert seen["seq_off"].tolist() == [0, 4, 6, 9, 13, 15, 17]
    assert seen["pair_a"].tolist() == [0, 1, 2] and seen["pair_b"].tolist() == [3, 4, 5]
    assert seen["pair_max_cost"].tolist() == [6, 2, 6] and seen["kw"] == {}
    assert seen["tables"].gap_open == 60
    assert isinstance(res, globalign_amd.BatchCounts)
    assert res.counts.dtype == np.float64 and res.counts.tolist() == [3.0, 2.0 ** 60, np.inf]
    assert res.exact.dtype == np.bool_ and res.exact.tolist() == [True, False, False]
    assert res.costs.tolist() == [0, 1, 2] and res.scores.tolist() == [4, 1, 1]
    assert res.gap_open_cost == 60 and res.gap_open_score == -60 and res.costing_mat["A"]["C"] == 6
    assert res.count(0) == 3 and type(res.count(0)) is int and type(res.count(1)) is float


# ---------------------------------------------------------------- the expected-count helper against the reference
def test_pinned_pairs_cover_the_asked_range():
    assert len(ac.PINNED) >= 6
    assert all(2 <= len(s) <= 8 for s1, s2, _ in ac.PINNED for s in (s1, s2))
    assert sum(c >= 2 for _, _, c in ac.PINNED) >= 3 and any(c >= 5 for _, _, c in ac.PINNED)


@pytest.mark.parametrize("s1,s2,count", ac.PINNED)
def test_helper_counts_what_the_reference_returns(s1, s2, count):
    """The int count of the recurrence is the number of different alignments the reference's traceback returns over
    the pinned seed range, and the float count is the same number."""
    cmat, o = ac.costs_of()
    assert ac.expected_count(s1, s2, cmat, o) == (count, float(count))
    assert ac.reference_distinct(s1, s2, cmat, o, ac.PINNED_SEEDS) == count


def test_helper_models_agree_and_grow():
    """Ints and floats agree while exact; a fully tied table grows past 2^53, where the float stays within the
    chain's rounding bound of the int."""
    cmat, o = ac.costs_of()
    rng = random.Random(3)
    for _ in range(20):
        s1 = "".join(rng.choice("ACGT") for _ in range(rng.randint(2, 30)))
        s2 = "".join(rng.choice("ACGT") for _ in range(rng.randint(2, 30)))
        ci, cf = ac.expected_count(s1, s2, cmat, o)
        assert ci >= 1 and ci < 2 ** 53 and cf == ci
    sets = np.full((40, 40), 0x1ff, dtype=np.int64)
    ci, cf = ac.count_from_sets(sets)
    assert ci > 2 ** 53 and abs(cf - ci) <= ci * 2 * 80 * 2.0 ** -53 * 1.01
    assert ac.count_from_sets(np.full((2, 2), 0x1ff, dtype=np.int64)) == (13, 13.0)


# ---------------------------------------------------------------- the host self-test
@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-s", "-C", CSRC, "batch_count_selftest", "batch_count_asan"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return True


@pytest.mark.parametrize("binary", ["ga_batch_count_selftest_asan", "ga_batch_count_selftest"])
def test_host_selftest(built, binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(LIB, binary)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
