"""GPU parity of GlobalAligner.match_support (ga_batch_support: batch_words_kernel fills a pair,
batch_support_table_kernel keeps the backward path counts N(i, j, 0), batch_flow_kernel runs the wavefront backwards for
the forward flows and multiplies, batch_support_gather_kernel makes the dense rows): every pair's (m, n) matrix bit for
bit against the pure-Python double model of tests/alignment_support.py, against its exact integers where the count is
below 2^53, counts and costs against count_alignments, on every route the engine has; and the tie-in with
enumerate_alignments, whose complete families tally to the same matrix."""
import math
import random

import numpy as np
import pytest

from tests import alignment_counts as ac
from tests import alignment_ranks as ar
from tests import alignment_support as asup
from tests.conftest import load_matrix, set_knob, splitmix_seq
from tests.test_gpu_batch_rank import PROTEIN_SHAPES, ROUTE_SHAPES, SHAPES

pytestmark = pytest.mark.gpu

BLOSUM = dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)
# every decision ties: mismatches at twice the gap extension, no gap open cost (pairs of unlike poly-letter sequences)
TIED = dict(mismatch_cost=2, gap_open_cost=0, gap_extension_cost=1)
NEW_BUFFERS = {"bm_table", "bm_toff", "bm_ooff", "bm_out", "bm_count", "bm_ticket"}


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


def _models(kw, pairs, blosum=None):
    """[(int count, ints, floats, float count)] of the pairs under the settings, by the pure-Python model."""
    out = []
    for s1, s2 in pairs:
        cmat, o = ac.costs_of(s1, s2, blosum=blosum, **kw)
        R = ar.ranked(s1.upper(), s2.upper(), cmat, o)
        out.append((R.count,) + asup.support_model(R))
    return out


def _check_support(ga, kw, pairs, want):
    """match_support(pairs) against the model: every matrix == the float model's, == the ints where the count is exact;
    the counts; count_alignments's counts and costs."""
    al = ga.GlobalAligner(max_seq_len_prod=None, **kw)
    A, B = [p[0] for p in pairs], [p[1] for p in pairs]
    res = al.match_support(A, B)
    assert isinstance(res, ga.BatchSupport) and len(res.support) == len(pairs)
    assert res.counts.dtype == np.float64 and res.counts.shape == (len(pairs),)
    assert res.exact.dtype == np.bool_ and np.array_equal(res.exact, res.counts < 2.0 ** 53)
    for k, (count, ints, floats, cf) in enumerate(want):
        got = res.support[k]
        assert got.dtype == np.float64 and got.shape == (len(A[k]), len(B[k])), k
        assert res.counts[k] == cf, (k, float(res.counts[k]), cf)
        bad = np.argwhere(~(got == floats))
        assert bad.size == 0, (k, got.shape, bad[:4].tolist(), [float(got[tuple(b)]) for b in bad[:4]],
                               [float(floats[tuple(b)]) for b in bad[:4]])
        assert not np.isnan(got).any() and (got >= 0).all() and (got <= res.counts[k]).all()
        if count < 2 ** 53:
            assert bool(res.exact[k]) and res.count(k) == count and got.tolist() == ints, k
            assert (got.sum(axis=1) <= count).all() and (got.sum(axis=0) <= count).all()
    assert res.seqs_1 == [a.upper() for a in A] and res.seqs_2 == [b.upper() for b in B]
    counted = al.count_alignments(A, B)
    assert np.array_equal(res.counts, counted.counts) and np.array_equal(res.costs, counted.costs)
    assert np.array_equal(res.scores, counted.scores) and res.costs.dtype == np.int64
    return res


@pytest.fixture(scope="module")
def dna_batch():
    """The parity shapes under the everyday DNA settings, with the model's supports."""
    rng = random.Random(2025)
    pairs = [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in SHAPES]
    return pairs, _models({}, pairs)


@pytest.fixture(scope="module")
def route_batch():
    rng = random.Random(4096)
    pairs = [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in ROUTE_SHAPES]
    return pairs, _models({}, pairs)


def test_parity_dna(ga, dna_batch):
    pairs, want = dna_batch
    assert len(pairs) == 19 and SHAPES[-1] == (1030, 515)
    # the last pair has its edge column in HBM and a count past 2^53: the doubles' order decides its bits
    assert want[-1][0] > 2 ** 64 and all(w[0] < 2 ** 28 for w in want[:-1]) and min(w[0] for w in want) == 1
    res = _check_support(ga, {}, pairs, want)
    info = _engine().batch_support_info()
    assert info["kernel_pairs"] == 19 and info["single_fill_pairs"] == 0 and info["fill_chunks"] == 1
    assert info["fill_launches"] == 1 and info["support_launches"] == 1 and info["hbm_edge_pairs"] == 1
    assert res.gap_open_cost == 4 and res.gap_open_score == -4
    assert res.exact.tolist() == [True] * 18 + [False]
    # a pair with one member: its columns are the whole core
    k = [w[0] for w in want].index(1)
    assert set(np.unique(res.support[k]).tolist()) <= {0.0, 1.0} and len(res.core(k)) == int(res.support[k].sum())


def test_parity_protein_blosum62(ga):
    """BLOSUM62, gap open 10: asymmetric gap costs, two-byte words."""
    pairs = [(splitmix_seq(m, 2 * k + 1, "protein"), splitmix_seq(n, 2 * k + 2, "protein"))
             for k, (m, n) in enumerate(PROTEIN_SHAPES)]
    _check_support(ga, BLOSUM, pairs, _models(BLOSUM, pairs, blosum=load_matrix("BLOSUM62")))
    assert _engine().batch_support_info()["kernel_pairs"] == 12


def test_fully_tied_small_shapes(ga):
    """Every decision tied on the small shapes: the largest flows a shape can have; past 2^53 the doubles' bits."""
    shapes = [(m, n) for m, n in SHAPES if m * n <= 64 * 65 + 64]
    assert (2, 2) in shapes and (64, 65) in shapes and (2, 129) in shapes and (1025, 3) in shapes and len(shapes) == 12
    pairs = [("A" * m, "C" * n) for m, n in shapes]
    want = _models(TIED, pairs)
    assert want[0][0] == 13 and max(w[0] for w in want) > 2 ** 100
    res = _check_support(ga, TIED, pairs, want)
    assert res.support[0].tolist() == want[0][1] and not res.exact.all() and np.isfinite(res.counts).all()


@pytest.mark.parametrize("o", [6, 7, 127])
def test_gap_open_widths(ga, o):
    """One-, two- and four-byte traceback words (tie_classes.tb_word_bytes: 1, 2, 4)."""
    from tests import tie_classes
    assert tie_classes.tb_word_bytes(o) == {6: 1, 7: 2, 127: 4}[o]
    rng = random.Random(100 + o)
    shapes = [(65, 129), (63, 257), (257, 64), (3, 65), (2, 2), (130, 520)]
    pairs = [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in shapes]
    kw = dict(match_score=3, mismatch_score=-2, gap_open_score=-o, gap_extension_score=-1)
    _check_support(ga, kw, pairs, _models(kw, pairs))


def test_routes_give_the_same_supports(ga, route_batch, monkeypatch):
    """The default route and the single-pair fill's words in their own layout: the same matrices and counts, and
    ga_batch_support_info shows the route taken."""
    pairs, want = route_batch
    base = _check_support(ga, {}, pairs, want)
    info = _engine().batch_support_info()
    assert info["kernel_pairs"] == 4 and info["single_fill_pairs"] == 0 and info["fill_chunks"] == 1
    assert info["hbm_edge_pairs"] == 1     # (1100, 520): two stripes, more rows than the LDS share
    set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", 4096)
    large = _check_support(ga, {}, pairs, want)
    info = _engine().batch_support_info()
    assert info["kernel_pairs"] == 0 and info["single_fill_pairs"] == 4 and info["support_launches"] == 4
    assert info["fill_launches"] == 4 and info["hbm_edge_pairs"] == 1
    assert all(np.array_equal(x, y) for x, y in zip(large.support, base.support))
    assert np.array_equal(large.counts, base.counts) and np.array_equal(large.costs, base.costs)
    # word widths on that route
    for o in (7, 127):
        kw = dict(match_score=3, mismatch_score=-2, gap_open_score=-o, gap_extension_score=-1)
        _check_support(ga, kw, pairs[:2], _models(kw, pairs[:2]))
        assert _engine().batch_support_info()["single_fill_pairs"] == 2
    monkeypatch.undo()
    _check_support(ga, {}, pairs[:1], want[:1])
    assert _engine().batch_support_info()["kernel_pairs"] == 1


@pytest.mark.parametrize("knob", ["GA_BATCH_SUPPORT_BYTES", "GA_BATCH_RANK_TABLE_BYTES", "GA_BATCH_SAMPLE_CHUNK_WORDS"])
def test_forced_chunking(ga, monkeypatch, knob):
    """Five pairs of 40 x 41 to 80 x 81 in more than one fill chunk, cut by the output's cap, the tables' cap (each set
    just above the largest pair's own) or the words' cap: the same matrices as the uncut batch."""
    rng = random.Random(55)
    pairs = [(_rand(rng, "ACGT", 40 + 10 * k), _rand(rng, "ACGT", 41 + 10 * k)) for k in range(5)]
    want = _models({}, pairs)
    base = _check_support(ga, {}, pairs, want)
    info = _engine().batch_support_info()
    assert info["fill_chunks"] == 1 and info["support_launches"] == 1 and info["kernel_pairs"] == 5
    value = {"GA_BATCH_SUPPORT_BYTES": 80 * 81 * 8 + 1, "GA_BATCH_RANK_TABLE_BYTES": (80 + 63) * 3 * 2 * 64 * 8 + 1,
             "GA_BATCH_SAMPLE_CHUNK_WORDS": 5200}[knob]
    set_knob(monkeypatch, knob, value)
    res = _check_support(ga, {}, pairs, want)
    info = _engine().batch_support_info()
    assert info["fill_chunks"] > 1 and info["support_launches"] == info["fill_chunks"] == info["fill_launches"]
    assert info["kernel_pairs"] == 5 and info["single_fill_pairs"] == 0
    assert all(np.array_equal(x, y) for x, y in zip(res.support, base.support))


def test_enumeration_tallies_to_the_support(ga):
    """Small pairs whose whole family enumerate_alignments lists: tallying its members' letter-letter columns gives
    `support` exactly, core(k)'s columns occur in every member, and column_support of a member is fraction(k) on its
    columns."""
    al = ga.GlobalAligner()
    rng = random.Random(3060)
    A = [p[0] for p in ac.PINNED] + [_rand(rng, "ACGT", rng.randint(30, 60)) for _ in range(12)]
    B = [p[1] for p in ac.PINNED] + [_rand(rng, "ACGT", rng.randint(30, 60)) for _ in range(12)]
    res = al.match_support(A, B)
    fam = al.enumerate_alignments(A, B)
    counted = al.count_alignments(A, B)
    assert np.array_equal(res.counts, counted.counts) and np.array_equal(res.costs, counted.costs)
    assert res.exact.all() and [res.count(k) for k in range(8)] == [p[2] for p in ac.PINNED]
    assert max(res.count(k) for k in range(len(A))) >= 10
    for k in range(len(A)):
        assert fam.complete(k) and int(fam.counts[k]) == res.count(k)
        members = list(zip(fam.seq_1_aligned[k], fam.seq_2_aligned[k]))
        assert res.support[k].tolist() == asup.tally_strings(len(A[k]), len(B[k]), members), k
        core = {tuple(x) for x in res.core(k).tolist()}
        for a, b in members[:50]:
            cols, i, j = [], 0, 0
            for x, y in zip(a, b):
                cols.append((i, j) if x != "-" and y != "-" else None)
                i += x != "-"
                j += y != "-"
            assert core <= set(cols)
            got = res.column_support(k, a, b)
            frac = res.fraction(k)
            assert all(got[c] == frac[ij] for c, ij in enumerate(cols) if ij is not None) and (got > 0).all()
        un1 = res.unaligned_1(k)
        assert un1.tolist() == [sum(1 for a, b in members if _faces_gap(a, b, i)) for i in range(len(A[k]))]


def _faces_gap(own, other, i):
    q = 0
    for x, y in zip(own, other):
        if x != "-":
            if q == i:
                return y == "-"
            q += 1
    raise AssertionError


def test_refusals(ga, monkeypatch):
    al = ga.GlobalAligner()
    s1, s2, _ = ac.PINNED[-1]
    with pytest.raises(ValueError) as e:
        al.match_support([s1, "A", "C"], [s2, s2, "G"])
    assert str(e.value) == "pair 1: match_support needs sequences of at least two letters"
    # the saturation case of the count tests: 450 x 450 fully tied counts to +inf
    tied = ga.GlobalAligner(**TIED)
    with pytest.raises(ValueError) as e:
        tied.match_support(["AC", "G" * 450, "G" * 450], ["GT", "T" * 450, "T" * 450])
    assert str(e.value) == "pair 1: the count of co-optimal alignments is not finite"
    assert tied.match_support(["AC"], ["GT"]).count(0) == 13
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner(traceback=False).match_support([s1], [s2])
    assert "match_support" in str(e.value)
    with pytest.raises(ValueError) as e:
        ga.GlobalAligner(devices=[0, 1]).match_support([s1], [s2])
    assert "one GPU" in str(e.value)
    # a pair whose own matrix exceeds the output's cap: refused before any launch, the lowest such pair
    set_knob(monkeypatch, "GA_BATCH_SUPPORT_BYTES", 8 * 5 * 8)
    with pytest.raises(ValueError) as e:
        al.match_support(["ACGTACGT", "ACGTACGTA", "ACGTACGTAC"], ["ACGGT", "ACGGT", "ACGGT"])
    assert str(e.value) == "pair 1: support matrix exceeds the support output budget"
    assert _engine().batch_support_info()["fill_launches"] == 0
    assert al.match_support(["ACGTACGT"], ["ACGGT"]).counts[0] >= 1
    monkeypatch.undo()
    assert math.isfinite(al.match_support([s1], [s2]).counts[0])


def test_random_state_is_left_alone(ga):
    random.seed(99)
    before = random.getstate()
    ga.GlobalAligner().match_support(["ACGTACGT", "AACC"], ["ACGGT", "CCAAT"])
    assert random.getstate() == before


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
    _check_support(ga, {}, pairs, want)
    info = _engine().batch_support_info()
    assert (info["kernel_pairs"], info["single_fill_pairs"]) == ((19, 0) if which == "parity" else (0, 4))
    rep = _engine().guard_report()
    assert rep["guard_bytes"] == 4096 and rep["violations"] == []
    listed = {b["name"] for b in rep["buffers"] if b["guarded"]}
    assert NEW_BUFFERS | {"bc_scratch"} <= listed
