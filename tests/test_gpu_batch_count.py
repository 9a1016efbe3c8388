"""GPU parity of GlobalAligner.count_alignments (ga_batch_count: batch_words_kernel fills a pair, batch_count_kernel
counts the paths of its traceback DAG from the words the fill left): counts bit for bit against the pure-Python
double model of tests/alignment_counts.py, exact counts against its integers, costs against score_pairs, on every
route the engine has; and the tie-in with sample_alignments, whose distinct alignments the count bounds."""
import math
import random

import numpy as np
import pytest

from tests import alignment_counts as ac
from tests.conftest import load_matrix, set_knob, splitmix_seq

pytestmark = pytest.mark.gpu

BLOSUM = dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)
# every decision ties: mismatches at twice the gap extension, no gap open cost (pairs of unlike poly-letter sequences)
TIED = dict(mismatch_cost=2, gap_open_cost=0, gap_extension_cost=1)
# lengths 2-8; n around the lane and stripe edges and one past every stripe-width step (64 T + 1, T = 1 .. 8; 513 is
# also the first n of two stripes, 1025 of three); every m of {2, 63, 64, 65, 200} on one, two and three stripes; and
# one pair of two stripes with more rows than the LDS share holds (1024), whose edge column goes through HBM
SHAPES = ([(2, 2), (2, 8), (8, 2), (3, 5), (5, 3), (4, 4), (6, 7), (7, 6), (8, 8), (2, 3), (5, 8), (8, 5)] +
          [(m, n) for k, n in enumerate([63, 64, 65, 127, 128, 129, 193, 257, 321, 385, 449, 513, 1025])
           for m in [(2, 63, 64, 65, 200)[k % 5]]] +
          [(200, 513), (65, 1025), (64, 513), (63, 641), (2, 513), (200, 65), (200, 129), (65, 64), (64, 65), (63, 63),
           (2, 1025), (200, 200), (129, 2), (1025, 3), (1030, 515)])
NEW_BUFFERS = {"bc_out", "bc_ticket"}


@pytest.fixture(scope="module")
def ga():
    import globalign_amd
    from globalign_amd import _native
    assert _native.device_count() >= 1
    return globalign_amd


def _engine():
    from globalign_amd import _native
    return _native.default_engine(0)


def _rand(rng, alpha, n):
    return "".join(rng.choice(alpha) for _ in range(n))


def _expect(kw, pairs, blosum=None):
    """[(int count, float count)] of the pairs under the settings, by the pure-Python model."""
    out = []
    for s1, s2 in pairs:
        cmat, o = ac.costs_of(s1, s2, blosum=blosum, **kw)
        out.append(ac.expected_count(s1.upper(), s2.upper(), cmat, o))
    return out


def _check_counts(ga, kw, pairs, want):
    """count_alignments(pairs) against the model's (int, float) counts `want` and score_pairs's costs."""
    al = ga.GlobalAligner(max_seq_len_prod=None, **kw)
    A, B = [p[0] for p in pairs], [p[1] for p in pairs]
    res = al.count_alignments(A, B)
    assert isinstance(res, ga.BatchCounts)
    assert res.counts.dtype == np.float64 and res.counts.shape == (len(pairs),)
    assert res.exact.dtype == np.bool_ and res.exact.shape == (len(pairs),)
    assert not np.isnan(res.counts).any() and (res.counts >= 1).all()
    floats = np.array([w[1] for w in want], dtype=np.float64)
    bad = np.flatnonzero(~(res.counts == floats))
    assert bad.size == 0, [(int(k), len(A[k]), len(B[k]), float(res.counts[k]), float(floats[k])) for k in bad[:8]]
    assert np.array_equal(res.exact, res.counts < 2.0 ** 53)
    for k in np.flatnonzero(res.exact):
        assert res.count(k) == want[k][0] and type(res.count(k)) is int, k
    scored = al.score_pairs(A, B)
    assert np.array_equal(res.costs, scored.costs) and np.array_equal(res.scores, scored.scores)
    assert res.costs.dtype == np.int64 and res.scores.dtype == np.int64
    return res


@pytest.fixture(scope="module")
def dna_batch():
    """The parity shapes under the everyday DNA settings, with the model's counts."""
    rng = random.Random(2024)
    pairs = [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in SHAPES]
    return pairs, _expect({}, pairs)


@pytest.fixture(scope="module")
def protein_batch():
    pairs = [(splitmix_seq(m, 2 * k + 1, "protein"), splitmix_seq(n, 2 * k + 2, "protein"))
             for k, (m, n) in enumerate(SHAPES)]
    return pairs, _expect(BLOSUM, pairs, blosum=load_matrix("BLOSUM62"))


@pytest.fixture(scope="module")
def route_batch():
    """Pairs for the route tests: a few stripe shapes, and (1100, 520), a pair on two stripes whose edge column has
    more rows than the 1024 the LDS share holds and goes through HBM -- (1024, 600) just fits the share, and
    (3000, 70), on one stripe, has no edge column at all."""
    rng = random.Random(4096)
    shapes = [(65, 129), (300, 257), (513, 513), (70, 1500), (3000, 70), (1100, 520), (1024, 600)]
    pairs = [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in shapes]
    return pairs, _expect({}, pairs)


def test_parity_dna(ga, dna_batch):
    pairs, want = dna_batch
    assert len(pairs) == 40
    res = _check_counts(ga, {}, pairs, want)
    info = _engine().batch_count_info()
    assert info["kernel_pairs"] == 40 and info["single_fill_pairs"] == 0 and info["fill_chunks"] == 1
    assert info["fill_launches"] == 1 and info["count_launches"] == 1 and info["hbm_edge_pairs"] == 1
    assert res.gap_open_cost == 4 and res.gap_open_score == -4
    assert max(w[0] for w in want) >= 2 ** 20     # the long pairs have many co-optimal alignments


def test_parity_protein_blosum62(ga, protein_batch):
    """BLOSUM62, gap open 10: asymmetric gap costs, two-byte words."""
    pairs, want = protein_batch
    _check_counts(ga, BLOSUM, pairs, want)
    assert _engine().batch_count_info()["kernel_pairs"] == 40


@pytest.mark.parametrize("o", [6, 7, 127])
def test_gap_open_widths(ga, o):
    """One-, two- and four-byte traceback words (tie_classes.tb_word_bytes: 1, 2, 4)."""
    from tests import tie_classes
    assert tie_classes.tb_word_bytes(o) == {6: 1, 7: 2, 127: 4}[o]
    rng = random.Random(100 + o)
    shapes = [(513, 513), (65, 129), (63, 257), (256, 255), (257, 64), (3, 65), (40, 90), (17, 5), (2, 2), (5, 600)]
    pairs = [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in shapes]
    kw = dict(match_score=3, mismatch_score=-2, gap_open_score=-o, gap_extension_score=-1)
    _check_counts(ga, kw, pairs, _expect(kw, pairs))


def test_routes_give_the_same_counts(ga, route_batch, monkeypatch):
    """The default route, several fill chunks, and the single-pair fill's words in their own layout: the same counts,
    and ga_batch_count_info shows the route taken."""
    pairs, want = route_batch
    base = _check_counts(ga, {}, pairs, want)
    info = _engine().batch_count_info()
    assert info["kernel_pairs"] == 7 and info["single_fill_pairs"] == 0 and info["fill_chunks"] == 1
    # (1100, 520) has two stripes and more rows than the LDS share: its edge goes through HBM; (1024, 600) just fits
    assert info["hbm_edge_pairs"] == 1
    set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", 4096)
    large = _check_counts(ga, {}, pairs, want)
    info = _engine().batch_count_info()
    assert info["kernel_pairs"] == 0 and info["single_fill_pairs"] == 7 and info["count_launches"] == 7
    assert info["fill_launches"] == 7 and info["hbm_edge_pairs"] == 1
    assert np.array_equal(large.counts, base.counts) and np.array_equal(large.costs, base.costs)
    # word widths on that route
    for o in (7, 127):
        kw = dict(match_score=3, mismatch_score=-2, gap_open_score=-o, gap_extension_score=-1)
        _check_counts(ga, kw, pairs[:3], _expect(kw, pairs[:3]))
        assert _engine().batch_count_info()["single_fill_pairs"] == 3
    monkeypatch.undo()
    again = _check_counts(ga, {}, pairs, want)
    assert _engine().batch_count_info()["kernel_pairs"] == 7 and np.array_equal(again.counts, base.counts)


def test_forced_chunking(ga, monkeypatch):
    """GA_BATCH_SAMPLE_CHUNK_WORDS=5200: a pair of 80 x 81 has a slice of 2560 words, so five pairs take several fill
    chunks, each with a count launch of its own."""
    rng = random.Random(55)
    pairs = [(_rand(rng, "ACGT", 40 + 10 * k), _rand(rng, "ACGT", 41 + 10 * k)) for k in range(5)]
    want = _expect({}, pairs)
    base = _check_counts(ga, {}, pairs, want)
    info = _engine().batch_count_info()
    assert info["fill_chunks"] == 1 and info["count_launches"] == 1 and info["kernel_pairs"] == 5
    set_knob(monkeypatch, "GA_BATCH_SAMPLE_CHUNK_WORDS", 5200)
    res = _check_counts(ga, {}, pairs, want)
    info = _engine().batch_count_info()
    assert info["fill_chunks"] > 1 and info["count_launches"] == info["fill_chunks"] == info["fill_launches"]
    assert info["kernel_pairs"] == 5 and info["single_fill_pairs"] == 0
    assert np.array_equal(res.counts, base.counts)


def test_large_and_saturating_counts(ga):
    """Unlike poly-letter sequences under settings where every decision ties (the int model: 300 x 300 has a count of
    759 bits, 450 x 450 one of 1140 bits): the first equals the float model bit for bit and lies within the rounding
    bound of the int count -- two additions a cell along a dependency chain of at most m + n cells --, the second is
    +inf."""
    pairs = [("A" * 300, "C" * 300), ("G" * 450, "T" * 450), ("AC", "GT")]
    want = _expect(TIED, pairs)
    assert 2 ** 600 < want[0][0] < 2 ** 1000 and want[0][0].bit_length() == 759
    assert want[1][0] > 2 ** 1024 and want[1][0].bit_length() == 1140 and want[1][1] == math.inf
    assert want[2] == (13, 13.0)
    res = _check_counts(ga, TIED, pairs, want)
    assert _engine().batch_count_info()["kernel_pairs"] == 3
    assert res.exact.tolist() == [False, False, True]
    got = float(res.counts[0])
    assert math.isfinite(got) and got == want[0][1]
    from fractions import Fraction
    rel = abs(Fraction(got) - want[0][0]) / want[0][0]
    assert rel <= Fraction(2 * 600 * 1.01) / 2 ** 53, float(rel)
    assert res.counts[1] == math.inf and not res.exact[1] and res.count(1) == math.inf
    assert res.count(2) == 13


def test_counts_bound_the_samples(ga):
    """The pinned tiny pairs: over the pinned seed range sample_alignments returns exactly counts[k] different
    alignments.  Random pairs of 30-60 letters with 64 samples each: never more than counts[k]."""
    al = ga.GlobalAligner()
    A, B = [p[0] for p in ac.PINNED], [p[1] for p in ac.PINNED]
    res = al.count_alignments(A, B)
    assert res.exact.all() and [res.count(k) for k in range(len(A))] == [p[2] for p in ac.PINNED]
    seeds = [list(ac.PINNED_SEEDS)] * len(A)
    sam = al.sample_alignments(A, B, seeds=seeds)
    assert [len(sam.distinct(k)) for k in range(len(A))] == [res.count(k) for k in range(len(A))]
    assert np.array_equal(sam.costs, res.costs)
    rng = random.Random(3060)
    A = [_rand(rng, "ACGT", rng.randint(30, 60)) for _ in range(20)]
    B = [_rand(rng, "ACGT", rng.randint(30, 60)) for _ in range(20)]
    res = al.count_alignments(A, B)
    sam = al.sample_alignments(A, B, samples=64, seeds=7)
    for k in range(20):
        assert 1 <= len(sam.distinct(k)) <= res.counts[k], k
    assert any(len(sam.distinct(k)) > 1 for k in range(20))


def test_random_state_is_left_alone(ga):
    random.seed(99)
    before = random.getstate()
    ga.GlobalAligner().count_alignments(["ACGTACGT", "AACC"], ["ACGGT", "CCAAT"])
    assert random.getstate() == before


def test_words_beyond_the_budget_are_refused(ga, monkeypatch):
    """A pair off the kernel route whose words the single-pair fill would band has no count: ValueError for the
    lowest such pair, before anything is launched."""
    rng = random.Random(8)
    pairs = [(_rand(rng, "ACGT", 30), _rand(rng, "ACGT", 30)), (_rand(rng, "ACGT", 200), _rand(rng, "ACGT", 100)),
             (_rand(rng, "ACGT", 300), _rand(rng, "ACGT", 100))]
    set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", 4096)
    set_knob(monkeypatch, "GA_TB_BAND_ROWS", 32)
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner().count_alignments([p[0] for p in pairs], [p[1] for p in pairs])
    assert str(e.value).startswith("pair 1: traceback words exceed the budget")


@pytest.mark.parametrize("which", ["parity", "large"])
def test_guards(ga, dna_batch, route_batch, monkeypatch, which):
    """The parity batch and the large route with guard bands on every device buffer: no kernel stores out of range
    (no GA_E_GUARD), and the call's own buffers are among the guarded ones."""
    set_knob(monkeypatch, "GA_GUARD_BYTES", 4096)
    if which == "parity":
        pairs, want = dna_batch
    else:
        pairs, want = route_batch
        set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", 4096)
    _check_counts(ga, {}, pairs, want)
    info = _engine().batch_count_info()
    assert (info["kernel_pairs"], info["single_fill_pairs"]) == ((40, 0) if which == "parity" else (0, 7))
    assert info["hbm_edge_pairs"] == 1
    rep = _engine().guard_report()
    assert rep["guard_bytes"] == 4096 and rep["violations"] == []
    listed = {b["name"] for b in rep["buffers"] if b["guarded"]}
    assert NEW_BUFFERS | {"bc_scratch"} <= listed
    assert ("bs_tb" in listed) == (which == "parity") and ("fb.tb" in listed or which == "parity")
