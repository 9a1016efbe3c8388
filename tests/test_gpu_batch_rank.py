"""GPU parity of GlobalAligner.alignments_by_rank, enumerate_alignments and sample_alignments_uniform (ga_batch_rank:
batch_words_kernel fills a pair, batch_rank_table_kernel keeps the saturating u64 path counts of every state,
batch_rank_walk_kernel unranks, one lane per walk): the three strings of every slot against the pure-Python exact-integer
model of tests/alignment_ranks.py, the counts against min(model count, 2^64 - 1), the costs against score_pairs, on
every route the engine has; and the tie-in with sample_alignments, whose draws are members of the enumeration."""
import random

import numpy as np
import pytest

from tests import alignment_counts as ac
from tests import alignment_ranks as ar
from tests.conftest import load_matrix, set_knob, splitmix_seq

pytestmark = pytest.mark.gpu

CAP = ar.CAP
BLOSUM = dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)
# every decision ties: mismatches at twice the gap extension, no gap open cost (pairs of unlike poly-letter sequences)
TIED = dict(mismatch_cost=2, gap_open_cost=0, gap_extension_cost=1)
# lane and stripe edges, one / two / three stripes, and (1030, 515): two stripes with more rows than the LDS share
# holds, so its edge column goes through HBM, and a count past 2^64, so it saturates
SHAPES = [(2, 2), (2, 8), (8, 2), (5, 3), (7, 6), (2, 63), (63, 64), (64, 65), (65, 127), (200, 128), (2, 129), (63, 513),
          (64, 1025), (200, 513), (65, 64), (129, 2), (1025, 3), (200, 200), (1030, 515)]
PROTEIN_SHAPES = [(2, 2), (5, 3), (7, 6), (2, 63), (63, 64), (64, 65), (65, 127), (200, 128), (2, 129), (63, 513),
                  (65, 64), (200, 200)]
ROUTE_SHAPES = [(65, 129), (300, 257), (1100, 520), (3000, 70)]
NEW_BUFFERS = {"br_table", "br_out", "br_items", "br_ticket"}


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
    out = []
    for s1, s2 in pairs:
        cmat, o = ac.costs_of(s1, s2, blosum=blosum, **kw)
        out.append(ar.ranked(s1.upper(), s2.upper(), cmat, o))
    return out


def _some_ranks(models, rng, drawn, extra=()):
    """Per pair: 0, 1, the last, the middle one and `drawn` seeded ranks, all below min(count, CAP); for a pair whose
    count saturates also `extra`."""
    out = []
    for R in models:
        lim = min(R.count, CAP)
        own = [0, min(1, lim - 1), lim - 1, lim // 2] + [rng.randrange(lim) for _ in range(drawn)]
        out.append(own + (list(extra) if R.count >= CAP else []))
    return out


def _check_ranked(ga, kw, pairs, models, ranks):
    """alignments_by_rank(pairs, ranks) against the models: every slot's three strings, the counts, saturated, and
    score_pairs's costs."""
    al = ga.GlobalAligner(max_seq_len_prod=None, **kw)
    A, B = [p[0] for p in pairs], [p[1] for p in pairs]
    res = al.alignments_by_rank(A, B, ranks)
    assert isinstance(res, ga.BatchRanked)
    assert res.counts.dtype == np.uint64 and res.counts.shape == (len(pairs),)
    assert [int(c) for c in res.counts] == [min(R.count, CAP) for R in models]
    assert res.saturated.dtype == np.bool_ and res.saturated.tolist() == [R.count >= CAP for R in models]
    for k, R in enumerate(models):
        assert res.ranks[k].dtype == np.uint64 and res.ranks[k].tolist() == list(ranks[k])
        assert len(res.seq_1_aligned[k]) == len(res.middle_part[k]) == len(res.seq_2_aligned[k]) == len(ranks[k])
        for t, r in enumerate(ranks[k]):
            got = (res.seq_1_aligned[k][t], res.middle_part[k][t], res.seq_2_aligned[k][t])
            assert got == R.strings(r), (k, R.m, R.n, r)
    scored = al.score_pairs(A, B)
    assert np.array_equal(res.costs, scored.costs) and np.array_equal(res.scores, scored.scores)
    assert res.costs.dtype == np.int64 and res.scores.dtype == np.int64
    return res


@pytest.fixture(scope="module")
def dna_batch():
    """The parity shapes under the everyday DNA settings, with their models and ranks."""
    rng = random.Random(2025)
    pairs = [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in SHAPES]
    models = _models({}, pairs)
    return pairs, models, _some_ranks(models, random.Random(77), 60, extra=(2 ** 64 - 2, 2 ** 63))


@pytest.fixture(scope="module")
def route_batch():
    rng = random.Random(4096)
    pairs = [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in ROUTE_SHAPES]
    models = _models({}, pairs)
    return pairs, models, _some_ranks(models, random.Random(78), 10)


def test_parity_dna(ga, dna_batch):
    pairs, models, ranks = dna_batch
    assert len(pairs) == 19 and all(len(r) >= 64 for r in ranks)
    counts = [R.count for R in models]
    assert min(counts) == 1 and counts[-1] > CAP and all(c < 2 ** 28 for c in counts[:-1])
    assert ranks[-1][-2:] == [2 ** 64 - 2, 2 ** 63]
    res = _check_ranked(ga, {}, pairs, models, ranks)
    info = _engine().batch_rank_info()
    assert info["kernel_pairs"] == 19 and info["single_fill_pairs"] == 0 and info["fill_chunks"] == 1
    assert info["fill_launches"] == 1 and info["table_launches"] == 1 and info["walk_launches"] == 1
    assert info["slots_walked"] == sum(len(r) for r in ranks) and info["saturated_pairs"] == 1
    assert res.saturated.tolist() == [False] * 18 + [True]
    assert res.gap_open_cost == 4 and res.gap_open_score == -4
    counted = ga.GlobalAligner(max_seq_len_prod=None).count_alignments([p[0] for p in pairs], [p[1] for p in pairs])
    for k in np.flatnonzero(counted.exact):
        assert int(res.counts[k]) == counted.count(k), k
    assert counted.exact[:18].all()


def test_parity_protein_blosum62(ga):
    """BLOSUM62, gap open 10: asymmetric gap costs, two-byte words."""
    pairs = [(splitmix_seq(m, 2 * k + 1, "protein"), splitmix_seq(n, 2 * k + 2, "protein"))
             for k, (m, n) in enumerate(PROTEIN_SHAPES)]
    models = _models(BLOSUM, pairs, blosum=load_matrix("BLOSUM62"))
    ranks = _some_ranks(models, random.Random(79), 16)
    assert len(pairs) == 12 and all(len(r) == 20 for r in ranks)
    _check_ranked(ga, BLOSUM, pairs, models, ranks)
    assert _engine().batch_rank_info()["kernel_pairs"] == 12


@pytest.mark.parametrize("o", [6, 7, 127])
def test_gap_open_widths(ga, o):
    """One-, two- and four-byte traceback words: the whole family where it has at most 256 members, else 32 ranks."""
    from tests import tie_classes
    assert tie_classes.tb_word_bytes(o) == {6: 1, 7: 2, 127: 4}[o]
    rng = random.Random(100 + o)
    shapes = [(65, 129), (63, 257), (257, 64), (3, 65), (2, 2)]
    pairs = [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in shapes]
    kw = dict(match_score=3, mismatch_score=-2, gap_open_score=-o, gap_extension_score=-1)
    models = _models(kw, pairs)
    ranks = [list(range(R.count)) if R.count <= 256 else [rng.randrange(min(R.count, CAP)) for _ in range(32)]
             for R in models]
    res = _check_ranked(ga, kw, pairs, models, ranks)
    for k, R in enumerate(models):
        assert res.complete(k) == (R.count <= 256)
        if R.count <= 256:
            assert len(set(zip(res.seq_1_aligned[k], res.middle_part[k], res.seq_2_aligned[k]))) == R.count


def test_enumeration_closes_the_loop_with_sampling(ga):
    al = ga.GlobalAligner()
    cmat, o = ac.costs_of()
    # the pinned tiny pairs: the enumeration is what the reference's tie-breaks reach over the pinned seeds
    A, B = [p[0] for p in ac.PINNED], [p[1] for p in ac.PINNED]
    res = al.enumerate_alignments(A, B)
    sam = al.sample_alignments(A, B, seeds=[list(ac.PINNED_SEEDS)] * len(A))
    for k, (s1, s2, count) in enumerate(ac.PINNED):
        assert res.complete(k) and int(res.counts[k]) == count
        triples = list(zip(res.seq_1_aligned[k], res.middle_part[k], res.seq_2_aligned[k]))
        assert len(set(triples)) == count and set(triples) == {key for key, _ in sam.distinct(k)}
        R = ar.ranked(s1, s2, cmat, o)
        assert triples == [R.strings(r) for r in range(count)]
    assert np.array_equal(sam.costs, res.costs)
    # random pairs of 30-60 letters: counts 4 .. 600, so the default limit completes them all
    rng = random.Random(3060)
    A = [_rand(rng, "ACGT", rng.randint(30, 60)) for _ in range(20)]
    B = [_rand(rng, "ACGT", rng.randint(30, 60)) for _ in range(20)]
    res = al.enumerate_alignments(A, B)
    sam = al.sample_alignments(A, B, samples=64, seeds=7)
    assert sorted(int(c) for c in res.counts)[::19] == [4, 600]
    for k in range(20):
        assert res.complete(k)
        family = set(zip(res.seq_1_aligned[k], res.middle_part[k], res.seq_2_aligned[k]))
        assert len(family) == int(res.counts[k]) == len(res.ranks[k])
        assert all(key in family for key, _ in sam.distinct(k)), k
    # every enumerated alignment costs what the pair costs
    for k in (0, 7, 19):
        cm, oo = ac.costs_of(A[k], B[k])
        for t in range(int(res.counts[k])):
            strings = (res.seq_1_aligned[k][t], res.middle_part[k][t], res.seq_2_aligned[k][t])
            assert ar.alignment_cost(strings, cm, oo) == int(res.costs[k]), (k, t)
        assert res.result(k, 0).cost == int(res.costs[k])
    # a limit below the count
    short = al.enumerate_alignments(A[:3], B[:3], limit=3)
    assert [len(r) for r in short.ranks] == [3, 3, 3] and not any(short.complete(k) for k in range(3))
    assert [short.seq_1_aligned[k] == res.seq_1_aligned[k][:3] for k in range(3)] == [True] * 3


def test_fully_tied_table(ga):
    pairs = [("A" * 300, "C" * 300), ("AC", "GT")]
    models = _models(TIED, pairs)
    assert models[0].count.bit_length() == 759 and models[1].count == 13
    res = _check_ranked(ga, TIED, pairs, models, [[0, 12345, 2 ** 64 - 2], list(range(13))])
    assert res.saturated.tolist() == [True, False] and int(res.counts[0]) == CAP
    assert res.complete(1) and not res.complete(0)
    assert len(set(zip(res.seq_1_aligned[1], res.middle_part[1], res.seq_2_aligned[1]))) == 13
    assert _engine().batch_rank_info()["saturated_pairs"] == 1


def test_routes_give_the_same_alignments(ga, route_batch, monkeypatch):
    """The default route and the single-pair fill's words in their own layout: the same strings and counts, and
    ga_batch_rank_info shows the route taken."""
    pairs, models, ranks = route_batch
    base = _check_ranked(ga, {}, pairs, models, ranks)
    info = _engine().batch_rank_info()
    assert info["kernel_pairs"] == 4 and info["single_fill_pairs"] == 0 and info["fill_chunks"] == 1
    set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", 4096)
    large = _check_ranked(ga, {}, pairs, models, ranks)
    info = _engine().batch_rank_info()
    assert info["kernel_pairs"] == 0 and info["single_fill_pairs"] == 4 and info["table_launches"] == 4
    assert info["fill_launches"] == 4 and info["walk_launches"] == 4
    assert info["slots_walked"] == sum(len(r) for r in ranks)
    assert np.array_equal(large.counts, base.counts) and np.array_equal(large.costs, base.costs)
    assert large.seq_1_aligned == base.seq_1_aligned and large.middle_part == base.middle_part
    assert large.seq_2_aligned == base.seq_2_aligned
    monkeypatch.undo()
    _check_ranked(ga, {}, pairs[:1], models[:1], ranks[:1])
    assert _engine().batch_rank_info()["kernel_pairs"] == 1


@pytest.mark.parametrize("knob", ["GA_BATCH_SAMPLE_CHUNK_WORDS", "GA_BATCH_RANK_TABLE_BYTES"])
def test_forced_chunking(ga, monkeypatch, knob):
    """Five pairs of 40 x 41 to 80 x 81 in more than one fill chunk, cut by the words' cap (a pair of 80 x 81 has a slice
    of 2560 words) or by the tables' cap, set just above the largest pair's table: a pair of m rows and n <= 128
    columns is one stripe at T = 2, (m + 63) * 3 * T * 64 entries of 8 bytes."""
    rng = random.Random(55)
    pairs = [(_rand(rng, "ACGT", 40 + 10 * k), _rand(rng, "ACGT", 41 + 10 * k)) for k in range(5)]
    models = _models({}, pairs)
    ranks = _some_ranks(models, random.Random(80), 8)
    base = _check_ranked(ga, {}, pairs, models, ranks)
    info = _engine().batch_rank_info()
    assert info["fill_chunks"] == 1 and info["table_launches"] == 1 and info["kernel_pairs"] == 5
    largest = max((m + 63) * 3 * 2 * 64 * 8 for m, _ in [(len(a), len(b)) for a, b in pairs])
    assert largest == (80 + 63) * 3 * 2 * 64 * 8
    set_knob(monkeypatch, knob, 5200 if knob == "GA_BATCH_SAMPLE_CHUNK_WORDS" else largest + 1)
    res = _check_ranked(ga, {}, pairs, models, ranks)
    info = _engine().batch_rank_info()
    assert info["fill_chunks"] > 1 and info["table_launches"] == info["fill_chunks"] == info["fill_launches"]
    assert info["kernel_pairs"] == 5 and info["single_fill_pairs"] == 0
    assert info["slots_walked"] == sum(len(r) for r in ranks)
    assert np.array_equal(res.counts, base.counts) and res.seq_1_aligned == base.seq_1_aligned


def test_refusals(ga, monkeypatch):
    al = ga.GlobalAligner()
    s1, s2, count = ac.PINNED[-1]
    with pytest.raises(ValueError) as e:
        al.alignments_by_rank([s1, s1], [s2, s2], [[0, count - 1], [3, count, count + 5]])
    assert str(e.value) == f"pair 1: rank {count} is not below the pair's count {count}"
    assert al.alignments_by_rank([s1], [s2], [[count - 1]]).seq_1_aligned[0] != []
    with pytest.raises(ValueError) as e:
        al.alignments_by_rank([s1, "A"], [s2, s2], [[0], [0]])
    assert str(e.value) == "pair 1: alignments_by_rank needs sequences of at least two letters"
    tied = ga.GlobalAligner(**TIED)
    with pytest.raises(ValueError) as e:
        tied.sample_alignments_uniform(["AC", "A" * 300], ["GT", "C" * 300], 3)
    assert str(e.value).startswith("pair 1: the count is saturated")
    assert tied.sample_alignments_uniform(["AC"], ["GT"], 3).counts.tolist() == [13]
    # a pair whose own table exceeds the tables' cap: refused before any launch, the lowest such pair
    set_knob(monkeypatch, "GA_BATCH_RANK_TABLE_BYTES", (8 + 63) * 3 * 64 * 8)
    with pytest.raises(ValueError) as e:
        al.alignments_by_rank(["ACGTACGT", "ACGTACGTA", "ACGTACGTAC"], ["ACGGT", "ACGGT", "ACGGT"], [[0], [0], [0]])
    assert str(e.value) == "pair 1: count table exceeds the rank table budget"
    assert al.alignments_by_rank(["ACGTACGT"], ["ACGGT"], [[0]]).counts[0] >= 1
    monkeypatch.undo()
    assert al.enumerate_alignments([s1], [s2]).complete(0)


def test_sample_alignments_uniform_is_alignments_by_rank_at_the_documented_ranks(ga):
    rng = random.Random(3060)
    A = [_rand(rng, "ACGT", rng.randint(30, 60)) for _ in range(6)]
    B = [_rand(rng, "ACGT", rng.randint(30, 60)) for _ in range(6)]
    al = ga.GlobalAligner()
    random.seed(99)
    before = random.getstate()
    uni = al.sample_alignments_uniform(A, B, [5, 1, 2, 3, 4, 6], seed=2026)
    counts = [int(c) for c in uni.counts]
    draw = random.Random(2026)
    want = [[draw.randrange(counts[k]) for _ in range(s)] for k, s in enumerate([5, 1, 2, 3, 4, 6])]
    assert [r.tolist() for r in uni.ranks] == want
    by_rank = al.alignments_by_rank(A, B, want)
    enum = al.enumerate_alignments(A, B)
    assert random.getstate() == before
    for line in ("seq_1_aligned", "middle_part", "seq_2_aligned"):
        assert getattr(uni, line) == getattr(by_rank, line)
        for k in range(6):
            assert getattr(uni, line)[k] == [getattr(enum, line)[k][r] for r in want[k]]
    assert np.array_equal(uni.counts, enum.counts) and np.array_equal(uni.costs, enum.costs)
    again = al.sample_alignments_uniform(A, B, [5, 1, 2, 3, 4, 6], seed=2026)
    assert again.seq_1_aligned == uni.seq_1_aligned


@pytest.mark.parametrize("which", ["parity", "large"])
def test_guards(ga, dna_batch, route_batch, monkeypatch, which):
    """The parity batch and the large route with guard bands on every device buffer: no kernel stores out of range
    (no GA_E_GUARD), and the call's own buffers are among the guarded ones."""
    set_knob(monkeypatch, "GA_GUARD_BYTES", 4096)
    if which == "parity":
        pairs, models, ranks = dna_batch
    else:
        pairs, models, ranks = route_batch
        set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", 4096)
    _check_ranked(ga, {}, pairs, models, ranks)
    info = _engine().batch_rank_info()
    assert (info["kernel_pairs"], info["single_fill_pairs"]) == ((19, 0) if which == "parity" else (0, 4))
    rep = _engine().guard_report()
    assert rep["guard_bytes"] == 4096 and rep["violations"] == []
    listed = {b["name"] for b in rep["buffers"] if b["guarded"]}
    assert NEW_BUFFERS | {"br_ranks", "br_toff", "bc_scratch"} <= listed
    assert ("bs_tb" in listed) == (which == "parity") and ("fb.tb" in listed or which == "parity")
