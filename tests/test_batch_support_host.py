"""GlobalAligner.match_support without a GPU: the exports, the validation and its order (count_alignments's, under this
method's name, all before any engine exists), the empty call, what the engine is handed, BatchSupport's methods on
hand-made instances, the host's share of ga_batch_support -- the support planner (globalign_amd/csrc/ga_batch.h
plan_batch_support) and the CPU model of the recurrence and of the wave's loop (ga_batch_support.h) -- in a stand-alone
self-test, plain and under AddressSanitizer + UndefinedBehaviorSanitizer, and the pure-Python expected support
(tests/alignment_support.py) pinned against a brute-force tally and against the reference's own traceback."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import alignment_counts as ac
from tests import alignment_ranks as ar
from tests import alignment_support as asup
from tests.conftest import ROOT, load_matrix

CSRC = os.path.join(ROOT, "globalign_amd", "csrc")
LIB = os.path.join(ROOT, "globalign_amd", "_lib")
BLOSUM = dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)
TIED = dict(mismatch_cost=2, gap_open_cost=0, gap_extension_cost=1)
PROTEIN = "ARNDCQEGHILKMFPSTWYV"


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
    assert "BatchSupport" in globalign_amd.__all__ and hasattr(globalign_amd, "BatchSupport")
    assert hasattr(globalign.GlobalAligner, "match_support")
    assert globalign_amd.BatchSupport._fields == ("support", "counts", "exact", "costs", "scores", "seqs_1", "seqs_2",
                                                  "scoring_mat", "costing_mat", "gap_open_score", "gap_open_cost")


def test_native_exports_the_new_entries():
    from globalign_amd import _native
    lib = _native.load_library()
    for name in ("ga_batch_support", "ga_batch_support_info", "ga_batch_support_timings"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "globalign_amd.h")).read()
    for name in ("ga_batch_support(", "ga_batch_support_info(", "ga_batch_support_timings(", "GA_E_COUNT"):
        assert name in header
    assert _native.GA_E_COUNT == -8


def test_validation_is_count_alignments_under_this_name(no_engine):
    ga = no_engine
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner().match_support(["ACGT", "AC"], ["ACGT"])
    assert "match_support needs as many first as second sequences" in str(e.value)
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner(traceback=False).match_support(["ACGT"], ["ACGT"])
    assert "match_support" in str(e.value) and "score_pairs" in str(e.value)
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner(devices=[0, 1]).match_support(["ACGT"], ["ACGT"])
    assert "match_support runs on one GPU" in str(e.value)
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner(traceback=False, devices=[0, 1]).match_support(["ACGT"], [])
    assert "as many first as second" in str(e.value)
    for bad in (["ACGT", "AC-T"], ["ACGT", ""]):
        with pytest.raises(RuntimeError) as e:
            ga.GlobalAligner().match_support(bad, ["ACGT", "ACGT"])
        with pytest.raises(RuntimeError) as want:
            ga.GlobalAligner().count_alignments(bad, ["ACGT", "ACGT"])
        assert str(e.value) == str(want.value)
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner().match_support(["ACGT"], ["ACЖT"])
    assert "latin-1" in str(e.value)
    with pytest.raises(TypeError):
        ga.GlobalAligner().match_support(["ACGT"], [5])
    # the sequences' own faults come before the two-letter rule, and that names the lowest pair
    with pytest.raises(RuntimeError):
        ga.GlobalAligner().match_support(["A", "AC-T"], ["ACGT", "ACGT"])
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner().match_support(["ACGT", "ACG", "A", "C"], ["ACGT", "T", "ACGT", "G"])
    assert str(e.value) == "pair 1: match_support needs sequences of at least two letters"


def test_empty_call(no_engine):
    ga = no_engine
    state = random.getstate()
    res = ga.GlobalAligner().match_support([], [])
    assert isinstance(res, ga.BatchSupport) and res.support == [] and res.seqs_1 == [] and res.seqs_2 == []
    assert res.counts.shape == (0,) and res.counts.dtype == np.float64
    assert res.exact.shape == (0,) and res.exact.dtype == np.bool_
    assert res.costs.shape == (0,) and res.scores.shape == (0,) and res.costs.dtype == np.int64
    assert res.scoring_mat is None and res.gap_open_cost == 4
    res = ga.GlobalAligner(**BLOSUM).match_support(iter([]), ())
    assert res.gap_open_cost == 10 and res.gap_open_score == -10 and res.costing_mat["A"]["-"] == 10
    with pytest.raises(ValueError):
        ga.GlobalAligner(traceback=False).match_support([], [])
    assert random.getstate() == state


class _Recorder:
    """An engine that records what batch_support is handed and answers with fixed costs, counts and supports."""

    def __init__(self, seen):
        self.seen = seen

    def batch_support(self, codes, seq_off, pair_a, pair_b, tables, pair_max_cost=None, **kw):
        self.seen.update(codes=codes, seq_off=seq_off, pair_a=pair_a, pair_b=pair_b, tables=tables,
                         pair_max_cost=pair_max_cost, kw=kw)
        lens = np.diff(seq_off)
        cells = lens[pair_a] * lens[pair_b]
        offsets = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
        return (np.arange(len(pair_a), dtype=np.int64), np.array([3.0, 2.0 ** 60, 5.0]), offsets,
                np.arange(int(offsets[-1]), dtype=np.float64))


def test_engine_gets_the_batch_and_the_result_is_cut_per_pair(monkeypatch):
    import globalign_amd
    from globalign_amd import _native
    seen = {}
    monkeypatch.setattr(_native, "default_engine", lambda device=0: _Recorder(seen))
    kw = dict(match_score=1, mismatch_score=-5, gap_open_score=-60, gap_extension_score=-1)
    state = random.getstate()
    res = globalign_amd.GlobalAligner(**kw).match_support(["acgt", "AA", "GGT"], ["ACGT", "AA", "TG"])
    assert random.getstate() == state
    assert len(seen["codes"]) == 17 and seen["seq_off"].tolist() == [0, 4, 6, 9, 13, 15, 17]
    assert seen["pair_a"].tolist() == [0, 1, 2] and seen["pair_b"].tolist() == [3, 4, 5]
    assert seen["pair_max_cost"].tolist() == [6, 2, 6] and seen["kw"] == {} and seen["tables"].gap_open == 60
    assert isinstance(res, globalign_amd.BatchSupport)
    assert [s.shape for s in res.support] == [(4, 4), (2, 2), (3, 2)] and all(s.dtype == np.float64 for s in res.support)
    assert res.support[0][1, 2] == 6.0 and res.support[1].tolist() == [[16.0, 17.0], [18.0, 19.0]]
    assert res.support[2][2, 1] == 25.0
    assert res.seqs_1 == ["ACGT", "AA", "GGT"] and res.seqs_2 == ["ACGT", "AA", "TG"]
    assert res.exact.tolist() == [True, False, True] and res.count(0) == 3 and type(res.count(1)) is float
    assert res.costs.tolist() == [0, 1, 2] and res.gap_open_cost == 60


def test_a_non_finite_count_is_a_value_error(monkeypatch):
    from globalign_amd import _native

    class Lib:
        @staticmethod
        def ga_last_error():
            return b"pair 1: the count of co-optimal alignments is not finite"

    monkeypatch.setattr(_native, "_lib", Lib)
    with pytest.raises(ValueError) as e:
        _native._check(_native.GA_E_COUNT)
    assert str(e.value) == "pair 1: the count of co-optimal alignments is not finite"


# ---------------------------------------------------------------- BatchSupport's methods
def _hand_made(support, counts, seqs_1, seqs_2):
    import globalign_amd
    counts = np.array(counts, dtype=np.float64)
    return globalign_amd.BatchSupport([np.array(s, dtype=np.float64) for s in support], counts, counts < 2.0 ** 53,
                                      np.zeros(len(counts), dtype=np.int64), np.zeros(len(counts), dtype=np.int64),
                                      list(seqs_1), list(seqs_2), None, None, -4, 4)


def test_methods_on_a_hand_made_instance():
    # "AC" against "AGC", 4 members: A-A in all of them, C-G in one, C-C in three; a second pair whose core is a path
    res = _hand_made([[[4, 0, 0], [0, 1, 3]], [[2, 0], [0, 2]]], [4, 2], ["AC", "GG"], ["AGC", "GG"])
    assert res.fraction(0).tolist() == [[1.0, 0.0, 0.0], [0.0, 0.25, 0.75]]
    core = res.core(0)
    assert core.dtype == np.int64 and core.tolist() == [[0, 0]] and res.core(1).tolist() == [[0, 0], [1, 1]]
    assert res.unaligned_1(0).tolist() == [0.0, 0.0] and res.unaligned_2(0).tolist() == [0.0, 3.0, 1.0]
    got = res.column_support(0, "A-C", "AGC")
    assert got.dtype == np.float64 and got.tolist() == [1.0, 0.75, 0.75]
    assert res.column_support(0, "AC-", "AGC").tolist() == [1.0, 0.25, 0.25]
    assert res.column_support(1, "GG", "GG").tolist() == [1.0, 1.0]
    for bad in (("A-C", "AGG"), ("AC", "AGC"), ("A-C", "AG"), ("A--C", "AG-C"), ("a-c", "AGC")):
        with pytest.raises(ValueError):
            res.column_support(0, *bad)
    empty = _hand_made([[[0, 0], [0, 0]]], [1], ["AA"], ["CC"])
    assert empty.core(0).shape == (0, 2) and empty.core(0).dtype == np.int64
    with pytest.raises(IndexError):
        res.fraction(2)


def test_column_support_on_every_rank_of_a_small_pair():
    """AGTTT / TATT, 7 members: every member's columns have a positive share, a column's share is the share of the
    members that have it, and the family's core columns have share 1 in every member."""
    s1, s2, count = "AGTTT", "TATT", 7
    cmat, o = ac.costs_of()
    R = ar.ranked(s1, s2, cmat, o)
    assert R.count == count
    ints, floats, cf = asup.support_model(R)
    res = _hand_made([floats], [cf], [s1], [s2])
    members = [R.strings(r) for r in range(count)]
    core = {tuple(x) for x in res.core(0).tolist()}
    for a, _, b in members:
        got = res.column_support(0, a, b)
        assert got.shape == (len(a),) and (got > 0).all() and (got <= 1).all()
        i = j = 0
        cols = set()
        for c, (x, y) in enumerate(zip(a, b)):
            if x != "-" and y != "-":
                share = sum(1 for aa, _, bb in members if (i, j) in _columns(aa, bb))
                assert got[c] == share / count
                cols.add((i, j))
            elif x == "-":
                assert got[c] == sum(1 for aa, _, bb in members if j in _gapped(bb, aa)) / count
            else:
                assert got[c] == sum(1 for aa, _, bb in members if i in _gapped(aa, bb)) / count
            i += x != "-"
            j += y != "-"
        assert core <= cols
    assert res.unaligned_1(0).tolist() == [count - sum(r) for r in ints]
    with pytest.raises(ValueError):
        res.column_support(0, "AGTTT", "TATT")


def _columns(a, b):
    out, i, j = set(), 0, 0
    for x, y in zip(a, b):
        if x != "-" and y != "-":
            out.add((i, j))
        i += x != "-"
        j += y != "-"
    return out


def _gapped(own, other):
    """The 0-based letters of `own` that face a gap in `other`."""
    out, i = set(), 0
    for x, y in zip(own, other):
        if x != "-" and y == "-":
            out.add(i)
        i += x != "-"
    return out


# ---------------------------------------------------------------- the model against brute force and the reference
def _small_pairs():
    """Seeded pairs of 2-9 letters under the three settings, with their Ranked; those with at most 5000 members."""
    rng = random.Random(915)
    blosum = load_matrix("BLOSUM62")
    out = []
    for _ in range(60):
        m, n = rng.randint(2, 9), rng.randint(2, 9)
        out.append(({}, "".join(rng.choice("ACGT") for _ in range(m)), "".join(rng.choice("ACGT") for _ in range(n)), None))
    for _ in range(30):
        m, n = rng.randint(2, 9), rng.randint(2, 9)
        out.append((BLOSUM, "".join(rng.choice(PROTEIN) for _ in range(m)), "".join(rng.choice(PROTEIN) for _ in range(n)),
                    blosum))
    for m in range(2, 8):
        for n in range(2, 8):
            out.append((TIED, "A" * m, "C" * n, None))
    models = []
    for kw, s1, s2, bl in out:
        cmat, o = ac.costs_of(s1, s2, blosum=bl, **kw)
        R = ar.ranked(s1, s2, cmat, o)
        if R.count <= 5000:
            models.append((kw is TIED, R))
    return models


@pytest.fixture(scope="module")
def small_models():
    return _small_pairs()


def test_forward_times_backward_is_the_brute_force_tally(small_models):
    assert len(small_models) >= 100 and sum(t for t, _ in small_models) >= 6
    assert max(R.count for _, R in small_models) >= 1000 and sum(R.count > 1 for _, R in small_models) >= 40
    for _, R in small_models:
        ints, floats, cf = asup.support_model(R)
        assert ints == asup.brute_force(R), (R.seq_1, R.seq_2)
        # the floats are the ints while the count is exact, and a row's and a column's supports sum to at most the count
        assert cf == R.count and floats.tolist() == ints
        assert all(sum(row) <= R.count for row in ints) and all(sum(col) <= R.count for col in zip(*ints))
        assert max(max(row) for row in ints) <= R.count


def test_floats_past_2_53_stay_close_and_sums_hold():
    cmat, o = ac.costs_of("A" * 45, "C" * 45, **TIED)
    R = ar.ranked("A" * 45, "C" * 45, cmat, o)
    assert R.count > 2 ** 53
    ints, floats, cf = asup.support_model(R)
    want = np.array(ints, dtype=object)
    rel = max(abs(int(floats[i, j]) - ints[i][j]) / max(ints[i][j], 1) for i in range(45) for j in range(45))
    assert rel <= 2 * 90 * 2.0 ** -53 * 1.01 and np.isfinite(floats).all()
    assert all(sum(row) <= R.count for row in ints) and all(sum(col) <= R.count for col in zip(*ints))
    assert want.shape == (45, 45)


@pytest.mark.parametrize("s1,s2,count", ac.PINNED)
def test_model_tallies_what_the_reference_returns(s1, s2, count):
    """The eight pairs test_batch_count_host.py pins: over seeds 0-399 the reference's traceback returns the pair's
    whole family (that test's pin), so the tally of its alignments' letter-letter columns is the model's support."""
    from oracle import core
    cmat, o = ac.costs_of()
    family = set()
    for s in ac.PINNED_SEEDS:
        words = np.array(random.Random(s).getstate()[1], dtype=np.uint32)
        got = core.align(s1, s2, cmat, o, words)
        assert got["status"] == "ok"
        family.add((got["strings"][0], got["strings"][2]))
    assert len(family) == count
    R = ar.ranked(s1, s2, cmat, o)
    ints, floats, cf = asup.support_model(R)
    assert ints == asup.tally_strings(len(s1), len(s2), family) and floats.tolist() == ints and cf == count


# ---------------------------------------------------------------- the host self-test
@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-s", "-C", CSRC, "batch_support_selftest", "batch_support_asan"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return True


@pytest.mark.parametrize("binary", ["ga_batch_support_selftest_asan", "ga_batch_support_selftest"])
def test_host_selftest(built, binary):
    """The recurrence against 128-bit integers and against a walk of every path, the wave's loop lane by lane (zero
    hand-over from columns past n, cell (m, n) in every lane and column of a lane) and plan_batch_support."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(LIB, binary)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
