"""The batched score-only calls without a GPU: GlobalAligner.score_pairs / score_matrix validate every pair as the
single call does, before any engine exists; and the batch planner (globalign_amd/csrc/ga_batch.h: work-list order,
routing, scratch sizing, the per-pair range guard) in a stand-alone self-test, plain and under AddressSanitizer +
UndefinedBehaviorSanitizer."""
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


def _single_error(ga, kw, s1, s2, **aligner):
    """The exception the single call raises for this pair (validation only: it never reaches the engine)."""
    with pytest.raises(Exception) as e:
        ga.GlobalAligner(traceback=False, **aligner, **kw).align(s1, s2)
    assert not isinstance(e.value, AssertionError)
    return e.value


def _same_error(got, want):
    assert type(got) is type(want) and str(got) == str(want)


def test_unequal_lists(no_engine):
    with pytest.raises(ValueError):
        no_engine.GlobalAligner().score_pairs(["ACGT", "AC"], ["ACGT"])


def test_dash_in_a_sequence(no_engine):
    ga = no_engine
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner().score_pairs(["ACGT", "AC-T", "A-"], ["ACGT", "ACGT", "ACGT"])
    _same_error(e.value, _single_error(ga, {}, "AC-T", "ACGT"))
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner().score_matrix(["ACGT", "ACGT"], ["AC", "A-C"])
    _same_error(e.value, _single_error(ga, {}, "ACGT", "A-C"))


def test_empty_sequence(no_engine):
    ga = no_engine
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner().score_pairs(["ACGT", "AC"], ["ACGT", ""])
    _same_error(e.value, _single_error(ga, {}, "AC", ""))
    assert "length 0" in str(e.value)


def test_max_seq_len_prod_names_the_lengths(no_engine):
    ga = no_engine
    a, b = "ACGT" * 5, "ACG" * 5
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner(max_seq_len_prod=300).score_pairs(["ACGT", a, a * 9], ["ACGT", b, b * 9])
    _same_error(e.value, _single_error(ga, {}, a, b, max_seq_len_prod=300))
    assert "20 and 15" in str(e.value)
    # the first offending pair in input order, whatever its fault: the empty pair comes before the long one
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner(max_seq_len_prod=300).score_pairs(["ACGT", "", a], ["ACGT", "A", b])
    assert "length 0" in str(e.value)


def test_letter_outside_blosum62(no_engine):
    ga = no_engine
    kw = dict(scoring_mat_name="BLOSUM62")
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner(**kw).score_pairs(["ARND", "ARND", "AU"], ["ARND", "AROD", "AR"])
    _same_error(e.value, _single_error(ga, kw, "ARND", "AROD"))
    # lower case is upper-cased first, as in the single call
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner(**kw).score_matrix(["arnd", "arod"])
    _same_error(e.value, _single_error(ga, kw, "arnd", "arod"))


def test_option_errors_come_once_and_first(no_engine):
    ga = no_engine
    kw = dict(match_score=2, mismatch_cost=5)
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner(**kw).score_pairs(["ACGT", "A-"], ["ACGT", "A"])
    _same_error(e.value, _single_error(ga, kw, "ACGT", "ACGT"))


def test_more_than_one_device(no_engine):
    with pytest.raises(ValueError):
        no_engine.GlobalAligner(devices=[0, 1]).score_pairs(["ACGT"], ["ACGT"])
    with pytest.raises(ValueError):
        no_engine.GlobalAligner(devices=[0, 1]).score_matrix(["ACGT"])


def test_empty_batch(no_engine):
    ga = no_engine
    state = random.getstate()
    res = ga.GlobalAligner().score_pairs([], [])
    assert isinstance(res, ga.BatchScores)
    assert res.costs.shape == (0,) and res.scores.shape == (0,)
    assert res.costs.dtype == np.int64 and res.scores.dtype == np.int64
    res = ga.GlobalAligner().score_matrix([])
    assert res.costs.shape == (0, 0) and res.scores.shape == (0, 0)
    res = ga.GlobalAligner().score_matrix(["ACGT", "AC"], [])
    assert res.costs.shape == (2, 0)
    assert random.getstate() == state


def test_empty_batch_still_checks_the_options(no_engine):
    ga = no_engine
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner(match_score=2, mismatch_cost=5).score_pairs([], [])
    _same_error(e.value, _single_error(ga, dict(match_score=2, mismatch_cost=5), "A", "A"))
    res = ga.GlobalAligner(scoring_mat_name="BLOSUM62", gap_open_score=-10).score_matrix([])
    assert res.gap_open_cost == 10 and res.gap_open_score == -10 and res.costing_mat["A"]["-"] == 10


def test_one_letter_pairs_get_their_own_max_cost(monkeypatch):
    """The engine is handed, per pair, the max_cost of the matrices the single call builds for that pair: those of a
    pair made of one letter hold no mismatch entry."""
    import globalign_amd
    from globalign_amd import _native
    from globalign_amd.scoring import get_max_val, validate_and_transform_args
    seen = {}

    class Recorder:
        def batch_costs(self, codes, seq_off, pair_a, pair_b, tables, pair_max_cost=None):
            seen.update(tables=tables, pair_max_cost=pair_max_cost)
            return np.zeros(len(pair_a), dtype=np.int64)

    monkeypatch.setattr(_native, "default_engine", lambda device=0: Recorder())
    kw = dict(match_score=1, mismatch_score=-5, gap_open_score=-60, gap_extension_score=-1)
    pairs = [("ACGT", "ACGT"), ("AAA", "AA"), ("aa", "AAAA"), ("AAA", "CC"), ("ACG", "A"), ("T", "TTT")]
    res = globalign_amd.GlobalAligner(**kw).score_pairs([p[0] for p in pairs], [p[1] for p in pairs])
    want = [get_max_val(validate_and_transform_args(None, None, a, b, **kw)[3]) for a, b in pairs]
    assert want == [6, 2, 2, 6, 6, 2]
    assert seen["pair_max_cost"].tolist() == want
    # scores of zero costs: n * floor(b / 2) + m * ceil(b / 2) with the pair's own b (here 1 either way)
    assert res.scores.tolist() == [4, 3, 2, 3, 3, 1]
    # a batch of one-letter pairs only is scored under pair 0's own tables: no per-pair array is needed
    globalign_amd.GlobalAligner(**kw).score_pairs(["AAA", "AA"], ["AA", "AAAAA"])
    assert seen["pair_max_cost"] is None and seen["tables"].max_cost == 2


# ---------------------------------------------------------------- the planner's self-test
@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-s", "-C", CSRC, "batch_selftest", "batch_asan"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return True


@pytest.mark.parametrize("binary", ["ga_batch_selftest_asan", "ga_batch_selftest"])
def test_planner_selftest(built, binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(LIB, binary)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
