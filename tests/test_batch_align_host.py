"""GlobalAligner.align_pairs without a GPU: the seeding that gives every pair a random stream of its own
(ga_debug_seed_state against CPython's random.seed), the seed and sequence validation, which finish before any engine
exists, and the host's share of ga_batch_align -- the align planner (globalign_amd/csrc/ga_batch.h), the per-pair
tie-break tables and the levels-to-strings decode (ga_batch_align.h) -- in a stand-alone self-test, plain, under
AddressSanitizer + UndefinedBehaviorSanitizer, and under ThreadSanitizer for the threaded table build."""
import ctypes as C
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


@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1])
def test_seed_state_matches_cpython(seed):
    from globalign_amd import _native
    lib = _native.load_library()
    out = np.zeros(625, dtype=np.uint32)
    assert lib.ga_debug_seed_state(seed, out.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert tuple(int(x) for x in out) == random.Random(seed).getstate()[1]


def test_seed_state_is_what_random_seed_leaves():
    from globalign_amd import _native
    lib = _native.load_library()
    out = np.zeros(625, dtype=np.uint32)
    before = random.getstate()
    try:
        random.seed(2 ** 40 + 7)
        want = random.getstate()[1]
    finally:
        random.setstate(before)
    assert lib.ga_debug_seed_state(2 ** 40 + 7, out.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert tuple(int(x) for x in out) == want


def test_unequal_lists(no_engine):
    with pytest.raises(ValueError):
        no_engine.GlobalAligner().align_pairs(["ACGT", "AC"], ["ACGT"])


def test_score_only_aligner_points_to_score_pairs(no_engine):
    with pytest.raises(ValueError) as e:
        no_engine.GlobalAligner(traceback=False).align_pairs(["ACGT"], ["ACGT"])
    assert "score_pairs" in str(e.value)


def test_more_than_one_device(no_engine):
    with pytest.raises(ValueError):
        no_engine.GlobalAligner(devices=[0, 1]).align_pairs(["ACGT"], ["ACGT"])


@pytest.mark.parametrize("seeds,error", [
    ([1], ValueError), ([1, 2, 3], ValueError),          # one seed per pair
    ([1, -1], ValueError), (-1, ValueError),             # negative
    ([0, 2 ** 64], ValueError), (2 ** 64, ValueError),   # too large
    (2 ** 64 - 1, ValueError),                           # base + 1 is too large
    ([1, 2.0], TypeError), (1.5, TypeError), ([1, "2"], TypeError), ("12", TypeError), (None, TypeError),
])
def test_bad_seeds(no_engine, seeds, error):
    with pytest.raises(error):
        no_engine.GlobalAligner().align_pairs(["ACGT", "AC"], ["ACGT", "AG"], seeds=seeds)


def test_seeds_are_checked_before_the_sequences(no_engine):
    with pytest.raises(ValueError) as e:
        no_engine.GlobalAligner().align_pairs(["ACGT", "A-"], ["ACGT", ""], seeds=[0, -5])
    assert "seed" in str(e.value)


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
        ga.GlobalAligner().align_pairs(["ACGT", "AC-T", "A-"], ["ACGT", "ACGT", "ACGT"], seeds=[5, 5, 2 ** 63])
    same(e.value, single_error("AC-T", "ACGT"))
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner().align_pairs(["ACGT", "AC"], ["ACGT", ""])
    same(e.value, single_error("AC", ""))
    a, b = "ACGT" * 5, "ACG" * 5
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner(max_seq_len_prod=300).align_pairs(["ACGT", a], ["ACGT", b], seeds=9)
    same(e.value, single_error(a, b, max_seq_len_prod=300))
    kw = dict(scoring_mat_name="BLOSUM62")
    with pytest.raises(RuntimeError) as e:
        ga.GlobalAligner(**kw).align_pairs(["ARND", "ARND"], ["ARND", "AROD"])
    same(e.value, single_error("ARND", "AROD", **kw))


def test_empty_batch(no_engine):
    ga = no_engine
    state = random.getstate()
    for seeds in (0, [], 2 ** 64 - 1):
        res = ga.GlobalAligner().align_pairs([], [], seeds=seeds)
        assert isinstance(res, ga.BatchAlignments)
        assert res.seq_1_aligned == [] and res.middle_part == [] and res.seq_2_aligned == []
        assert res.costs.shape == (0,) and res.scores.shape == (0,)
        assert res.costs.dtype == np.int64 and res.scores.dtype == np.int64
    res = ga.GlobalAligner(scoring_mat_name="BLOSUM62", gap_open_score=-10).align_pairs([], [])
    assert res.gap_open_cost == 10 and res.gap_open_score == -10 and res.costing_mat["A"]["-"] == 10
    with pytest.raises(ValueError):
        ga.GlobalAligner().align_pairs([], [], seeds=[1])
    with pytest.raises(ValueError):
        ga.GlobalAligner().align_pairs([], [], seeds=-1)
    assert random.getstate() == state


def test_result_method():
    import globalign_amd
    res = globalign_amd.BatchAlignments(["AC-T", "A"], ["|| |", "*"], ["ACGT", "C"], np.array([3, 5]), np.array([4, -3]),
                                        {"A": {}}, {"C": {}}, -4, 4)
    r = res.result(1)
    assert isinstance(r, globalign_amd.AlignmentResults)
    assert r == globalign_amd.AlignmentResults("A", "*", "C", 5, -3, {"A": {}}, {"C": {}}, -4, 4, None)
    assert type(r.cost) is int and type(r.score) is int


def test_engine_gets_seeds_characters_and_own_max_cost(monkeypatch):
    """The engine is handed base + k as pair k's seed, the upper-cased characters beside the codes, and score_pairs's
    per-pair max_cost for one-letter pairs; the strings are cut from its buffers at its offsets."""
    import globalign_amd
    from globalign_amd import _native
    seen = {}

    class Recorder:
        def batch_align(self, codes, seq_off, pair_a, pair_b, tables, seeds, chars, pair_max_cost=None):
            seen.update(codes=codes, seq_off=seq_off, seeds=seeds, chars=bytes(chars), pair_max_cost=pair_max_cost)
            P = len(pair_a)
            bufs = tuple(np.frombuffer(t, dtype=np.uint8) for t in (b"AC-TxxAA", b"|| |yy* ", b"ACGTzzC-"))
            return (np.arange(P, dtype=np.int64), np.zeros(P, dtype=np.int32), np.array([4, 2], dtype=np.int64),
                    np.array([0, 6, 8], dtype=np.int64), bufs)

    monkeypatch.setattr(_native, "default_engine", lambda device=0: Recorder())
    kw = dict(match_score=1, mismatch_score=-5, gap_open_score=-60, gap_extension_score=-1)
    state = random.getstate()
    res = globalign_amd.GlobalAligner(**kw).align_pairs(["acgt", "AA"], ["ACGT", "A"], seeds=2 ** 64 - 2)
    assert random.getstate() == state
    assert seen["seeds"].dtype == np.uint64 and seen["seeds"].tolist() == [2 ** 64 - 2, 2 ** 64 - 1]
    assert seen["chars"] == b"ACGTAAACGTA" and len(seen["codes"]) == 11 and seen["seq_off"].tolist() == [0, 4, 6, 10, 11]
    assert seen["pair_max_cost"].tolist() == [6, 2]
    assert res.seq_1_aligned == ["AC-T", "AA"] and res.middle_part == ["|| |", "* "] and res.seq_2_aligned == ["ACGT", "C-"]
    assert res.costs.tolist() == [0, 1] and res.scores.tolist() == [4, 1]
    res = globalign_amd.GlobalAligner(**kw).align_pairs(["acgt", "AA"], ["ACGT", "A"], seeds=[7, 7])
    assert seen["seeds"].tolist() == [7, 7]


def test_index_error_names_the_lowest_pair(monkeypatch):
    import globalign_amd
    from globalign_amd import _native

    class Failing:
        def batch_align(self, codes, seq_off, pair_a, pair_b, tables, seeds, chars, pair_max_cost=None):
            P = len(pair_a)
            status = np.array([0, 1, 0, 1], dtype=np.int32)
            return (np.zeros(P, dtype=np.int64), status, np.zeros(P, dtype=np.int64), np.zeros(P + 1, dtype=np.int64),
                    tuple(np.zeros(1, dtype=np.uint8) for _ in range(3)))

    monkeypatch.setattr(_native, "default_engine", lambda device=0: Failing())
    with pytest.raises(IndexError) as e:
        globalign_amd.GlobalAligner().align_pairs(["AC", "A", "AC", "A"], ["AC", "ACGT", "AC", "ACGT"])
    assert str(e.value) == "pair 1: string index out of range"


# ---------------------------------------------------------------- the host self-test
@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-s", "-C", CSRC, "batch_align_selftest", "batch_align_asan", "batch_align_tsan"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return True


@pytest.mark.parametrize("binary", ["ga_batch_align_selftest_asan", "ga_batch_align_selftest_tsan",
                                    "ga_batch_align_selftest"])
def test_host_selftest(built, binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(LIB, binary)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "ThreadSanitizer" not in r.stderr
