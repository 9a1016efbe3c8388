"""GPU parity of the batched score-only calls (GlobalAligner.score_pairs / score_matrix, ga_batch_costs): every
cost against the CPU oracle's boundary + score fill with the pair's own sentinel big = (max_cost + 1) * max(m, n),
every score against the oracle's transform; a few pairs also against the single-pair call."""
import random

import numpy as np
import pytest

from tests.conftest import load_matrix, set_knob, splitmix_seq, state_digest

pytestmark = pytest.mark.gpu

DNA = dict(match_score=2, mismatch_score=-3, gap_open_score=-5, gap_extension_score=-1)
EDGE_LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513]


@pytest.fixture(scope="module")
def ga():
    import globalign_amd
    from globalign_amd import _native
    assert _native.device_count() >= 1
    return globalign_amd


def _rand(rng, alpha, n):
    return "".join(rng.choice(alpha) for _ in range(n))


def _oracle(kw, s1, s2, blosum=None, mtx=None):
    """(cost, score) of one pair: oracle.core.boundary + fill_score, min of the last cell."""
    from oracle import core, transform
    a1, a2, smat, cmat, _, goc = transform.settings(dict(kw, seq_1=s1, seq_2=s2), blosum=blosum, mtx=mtx)
    tab = core.Tables(cmat)
    a, b = tab.codes(a1), tab.codes(a2)
    big = (tab.max_cost + 1) * max(len(a), len(b))
    row0, col0 = core.boundary(tab, a, b, goc, big)
    cost = int(min(core.fill_score(tab, a, b, goc, row0, col0)))
    return cost, transform.cost_to_score(cost, len(a), len(b), transform.max_val(smat))


def _oracle_arrays(kw, pairs, **tables):
    ref = [_oracle(kw, s1, s2, **tables) for s1, s2 in pairs]
    return np.array([c for c, _ in ref], dtype=np.int64), np.array([s for _, s in ref], dtype=np.int64)


def _check_pairs(ga, kw, pairs, **tables):
    res = ga.GlobalAligner(max_seq_len_prod=None, **kw).score_pairs([p[0] for p in pairs], [p[1] for p in pairs])
    costs, scores = _oracle_arrays(kw, pairs, **tables)
    assert res.costs.dtype == np.int64 and res.scores.dtype == np.int64
    assert res.costs.shape == (len(pairs),) and res.scores.shape == (len(pairs),)
    bad = np.nonzero(res.costs != costs)[0]
    assert bad.size == 0, [(int(k), len(pairs[k][0]), len(pairs[k][1]), int(res.costs[k]), int(costs[k])) for k in bad[:8]]
    assert np.array_equal(res.scores, scores)
    return res


def _edge_pairs(rng, count):
    """Pairs over EDGE_LENGTHS: the corners first (length 1 on either side, m < 64, one / partial / several stripes),
    then mixed draws."""
    shapes = [(1, 1), (1, 513), (513, 1), (513, 513), (2, 300), (300, 3), (64, 64), (65, 129), (63, 257), (256, 255),
              (257, 64), (3, 65), (128, 128), (129, 127), (127, 513), (300, 300)]
    while len(shapes) < count:
        shapes.append((rng.choice(EDGE_LENGTHS), rng.choice(EDGE_LENGTHS)))
    return [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in shapes[:count]]


def test_stripe_edges_dna(ga):
    """Partial and multiple stripes, m < 64, length 1 on either side; 8 of the pairs also against the single call."""
    rng = random.Random(11)
    pairs = _edge_pairs(rng, 80)
    res = _check_pairs(ga, DNA, pairs)
    single = ga.GlobalAligner(max_seq_len_prod=None, traceback=False, **DNA)
    for k in (0, 1, 2, 3, 5, 9, 30, 79):
        r = single.align(*pairs[k])
        assert (r.cost, r.score) == (int(res.costs[k]), int(res.scores[k])), k
    assert res.gap_open_cost == 5 and res.gap_open_score == -5
    assert res.costing_mat["A"]["C"] == r.costing_mat["A"]["C"] and res.costing_mat["A"]["-"] == r.costing_mat["A"]["-"]


@pytest.mark.parametrize("o", [0, 7, 300])
def test_gap_open_widths(ga, o):
    rng = random.Random(100 + o)
    _check_pairs(ga, dict(match_score=3, mismatch_score=-2, gap_open_score=-o, gap_extension_score=-1),
                 _edge_pairs(rng, 20))


def test_protein_blosum62(ga):
    """BLOSUM62, gap open 10: gH = 9 and gV = 10 (asymmetric), int8 profile; lengths 30-700."""
    rng = random.Random(62)
    pairs = [(splitmix_seq(rng.randint(30, 700), 2 * k + 1, "protein"), splitmix_seq(rng.randint(30, 700), 2 * k + 2, "protein"))
             for k in range(40)]
    _check_pairs(ga, dict(scoring_mat_name="BLOSUM62", gap_open_score=-10), pairs, blosum=load_matrix("BLOSUM62"))


def test_matrix_file_int16_profile(ga, tmp_path):
    """A scoring matrix from a file whose sub' = sub - gV - gH needs the int16 profile (match: 0 - 200 - 200)."""
    letters = ["A", "C", "G", "T", "-"]
    scores = [[200 if x == y else -100 if "-" in (x, y) else -200 for y in letters] for x in letters]
    path = tmp_path / "wide.mtx"
    path.write_text("\n".join(["  ".join(letters)] + [letters[i] + " " + " ".join(str(v) for v in scores[i])
                                                      for i in range(len(letters))]) + "\n")
    from oracle import transform
    rng = random.Random(16)
    pairs = _edge_pairs(rng, 20)
    _check_pairs(ga, dict(scoring_mat_path=str(path), gap_open_score=-3), pairs,
                 mtx=transform.read_mtx_rows(letters, scores))


def test_sentinel_leak_batches(ga):
    """The 40 pairs of test_gpu_parity.test_sentinel_leak_cases (lengths 2-9, gap open 20 / 40 / 60), one batch per
    gap-open value: the finite big leaks into the optimum, so a big that is not the pair's own shows here."""
    rng = random.Random(5)
    by_open = {20: [], 40: [], 60: []}
    for _ in range(40):
        s1, s2 = _rand(rng, "ACGT", rng.randint(2, 9)), _rand(rng, "ACGT", rng.randint(2, 9))
        by_open[rng.choice([20, 40, 60])].append((s1, s2))
    assert sum(len(v) for v in by_open.values()) == 40
    for o, pairs in by_open.items():
        _check_pairs(ga, dict(match_score=1, mismatch_score=-1, gap_open_score=-o, gap_extension_score=-1), pairs)


@pytest.mark.parametrize("kw", [dict(match_score=1, mismatch_score=-5, gap_extension_score=-1),
                                dict(mismatch_cost=9, gap_extension_cost=1)], ids=["scores", "costs"])
@pytest.mark.parametrize("o", [20, 40, 60])
def test_one_letter_pairs_in_a_mixed_batch(ga, kw, o):
    """A pair made of one letter: the single call's match / mismatch matrices over that letter alone hold no mismatch
    entry, so max_cost -- and the sentinel big that leaks into the optimum at these gap-open costs -- is smaller than
    under the batch's union alphabet ('AAA' vs 'AA' at match 1 / mismatch -5 / open -60: cost 9, and 21 with the
    ACGT maximum).  Such pairs of unequal length, mixed with ordinary ones: every cost and score against the oracle
    and against align."""
    kw = dict(kw, **({"gap_open_score": -o} if "match_score" in kw else {"gap_open_cost": o}))
    rng = random.Random(o)
    pairs = [("ACGT", "ACGT"), ("AAA", "AA"), ("AAAAA", "AA"), ("aa", "AAAAAAA"), ("C", "CCCC"), ("TTTTTTTTT", "TT"),
             ("AAA", "CC"), ("ACG", "A"), ("G" * 70, "G" * 3), ("G" * 2, "G" * 130)]
    pairs += [(_rand(rng, "ACGT", rng.randint(2, 9)), _rand(rng, "ACGT", rng.randint(2, 9))) for _ in range(10)]
    res = _check_pairs(ga, kw, pairs)
    single = ga.GlobalAligner(traceback=False, **kw)
    for k in range(10):
        r = single.align(*pairs[k])
        assert (r.cost, r.score) == (int(res.costs[k]), int(res.scores[k])), (k, pairs[k])
    # one-letter pairs alone (pair 0's own tables serve all), and one of them first in a mixed batch
    _check_pairs(ga, kw, pairs[1:6])
    _check_pairs(ga, kw, [pairs[1], pairs[0], pairs[4]])


def test_one_letter_pairs_single_route(ga, monkeypatch):
    set_knob(monkeypatch, "GA_BATCH_MAX_CELLS", 0)
    kw = dict(match_score=1, mismatch_score=-5, gap_open_score=-60, gap_extension_score=-1)
    _check_pairs(ga, kw, [("ACGT", "ACGT"), ("AAA", "AA"), ("AAAAA", "AA"), ("AAA", "CC")])


def test_thin_and_long(ga):
    """One row / one column, and many stripes with the edge column in use (m above and below the LDS share)."""
    rng = random.Random(7)
    shapes = [(1, 3000), (3000, 1), (70, 5000), (5000, 70)]
    _check_pairs(ga, DNA, [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in shapes])


def test_long_rows_several_stripes(ga):
    """More rows than a wave's LDS edge column holds and more than one stripe: the HBM edge scratch, two pairs with
    different m sharing the slices."""
    rng = random.Random(8)
    shapes = [(1100, 600), (1025, 1030), (1024, 513), (40, 40)]
    _check_pairs(ga, DNA, [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in shapes])


def test_more_pairs_than_waves(ga):
    """6000 pairs of lengths 8-40: every resident wave takes several tickets; costs come back in input order."""
    rng = random.Random(6000)
    pairs = [(_rand(rng, "ACGT", rng.randint(8, 40)), _rand(rng, "ACGT", rng.randint(8, 40))) for _ in range(6000)]
    _check_pairs(ga, DNA, pairs)


def test_score_matrix(ga):
    rng = random.Random(12)
    seqs = [_rand(rng, "ACGT", L) for L in (1, 5, 40, 63, 64, 65, 100, 130, 200, 257, 300, 520)]
    res = ga.GlobalAligner(max_seq_len_prod=None, **DNA).score_matrix(seqs)
    costs, scores = _oracle_arrays(DNA, [(x, y) for x in seqs for y in seqs])
    assert res.costs.shape == (12, 12) and res.scores.shape == (12, 12)
    assert np.array_equal(res.costs, costs.reshape(12, 12)) and np.array_equal(res.scores, scores.reshape(12, 12))
    other = [_rand(rng, "ACGT", L) for L in (7, 90, 300)]
    res = ga.GlobalAligner(max_seq_len_prod=None, **DNA).score_matrix(seqs[:5], other)
    costs, scores = _oracle_arrays(DNA, [(x, y) for x in seqs[:5] for y in other])
    assert res.costs.shape == (5, 3)
    assert np.array_equal(res.costs, costs.reshape(5, 3)) and np.array_equal(res.scores, scores.reshape(5, 3))


def test_score_matrix_is_not_symmetric(ga):
    """BLOSUM62's costs have gH = 9 and gV = 10: [i][j] != [j][i] for sequences of different lengths."""
    kw = dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)
    seqs = [splitmix_seq(L, 40 + L, "protein") for L in (20, 55, 90, 200)]
    res = ga.GlobalAligner(**kw).score_matrix(seqs)
    costs, _ = _oracle_arrays(kw, [(x, y) for x in seqs for y in seqs], blosum=load_matrix("BLOSUM62"))
    costs = costs.reshape(4, 4)
    assert np.array_equal(res.costs, costs)
    assert any(costs[i][j] != costs[j][i] for i in range(4) for j in range(i))


def test_routing_gives_identical_arrays(ga, monkeypatch):
    """Mixed routes (GA_BATCH_MAX_CELLS=20000), every pair through the single-pair fill (0) and the default: the
    same arrays, equal to the oracle, in input order."""
    rng = random.Random(20000)
    pairs = [(_rand(rng, "ACGT", rng.randint(50, 600)), _rand(rng, "ACGT", rng.randint(50, 600))) for _ in range(24)]
    cells = [len(a) * len(b) for a, b in pairs]
    assert min(cells) <= 20000 < max(cells)
    costs, scores = _oracle_arrays(DNA, pairs)
    for limit in (20000, 0, None):
        if limit is not None:
            set_knob(monkeypatch, "GA_BATCH_MAX_CELLS", limit)
        res = ga.GlobalAligner(**DNA).score_pairs([p[0] for p in pairs], [p[1] for p in pairs])
        assert np.array_equal(res.costs, costs) and np.array_equal(res.scores, scores), limit
        monkeypatch.undo()


def test_state_between_calls(ga):
    """Two different batches back to back on one engine; a find_global_alignment call before and after a batch
    returns what it returns without it, with the same random state; the batch calls leave random alone."""
    rng = random.Random(9)
    first = [(_rand(rng, "ACGT", rng.randint(30, 400)), _rand(rng, "ACGT", rng.randint(30, 400))) for _ in range(50)]
    second = [(_rand(rng, "ACGT", rng.randint(5, 90)), _rand(rng, "ACGT", rng.randint(5, 90))) for _ in range(9)]
    x, y = _rand(rng, "ACGT", 150), _rand(rng, "ACGT", 170)

    def two_calls(between):
        random.seed(4)
        r1 = ga.find_global_alignment(seq_1=x, seq_2=y, **DNA)
        between()
        r2 = ga.find_global_alignment(seq_1=x, seq_2=y, **DNA)
        return r1[:5], r2[:5], state_digest()

    def batches():
        before = random.getstate()
        _check_pairs(ga, DNA, first)
        _check_pairs(ga, DNA, second)
        ga.GlobalAligner(**DNA).score_matrix([p[0] for p in second])
        assert random.getstate() == before

    assert two_calls(batches) == two_calls(lambda: None)


def test_range_guard_per_pair(ga):
    """mismatch cost 10^6: a 3 x 3 pair is in range, a 100 x 100 pair is not (big = 10^8 and 202 * 3 * 10^6 give a
    bound of 7 * 10^8, and four times that exceeds 2^31).  The batch of both fails as the single call fails for the
    second pair, naming pair 1; the 3 x 3 pair alone succeeds."""
    kw = dict(mismatch_cost=10 ** 6, gap_open_cost=1, gap_extension_cost=1)
    rng = random.Random(10)
    small = (_rand(rng, "ACGT", 3), _rand(rng, "ACGT", 3))
    large = (_rand(rng, "ACGT", 100), _rand(rng, "ACGT", 100))
    with pytest.raises(Exception) as single:
        ga.GlobalAligner(traceback=False, **kw).align(*large)
    with pytest.raises(Exception) as batch:
        ga.GlobalAligner(**kw).score_pairs([small[0], large[0]], [small[1], large[1]])
    assert type(batch.value) is type(single.value)
    assert "pair 1" in str(batch.value) and "int32 score range" in str(batch.value)
    assert "int32 score range" in str(single.value)
    _check_pairs(ga, kw, [small])
