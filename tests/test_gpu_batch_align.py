"""GPU parity of GlobalAligner.align_pairs (ga_batch_align, batch_align_kernel): pair k's strings and cost against the
CPU oracle's alignment from the state random.seed(s_k) leaves, its score against the oracle's transform; a few pairs
also against random.seed(s_k) followed by the single call."""
import random

import numpy as np
import pytest

from tests.conftest import load_matrix, set_knob, splitmix_seq, state_digest

pytestmark = pytest.mark.gpu

DNA = dict(match_score=2, mismatch_score=-3, gap_open_score=-5, gap_extension_score=-1)
EDGE_LENGTHS = [2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513]


@pytest.fixture(scope="module")
def ga():
    import globalign_amd
    from globalign_amd import _native
    assert _native.device_count() >= 1
    return globalign_amd


def _rand(rng, alpha, n):
    return "".join(rng.choice(alpha) for _ in range(n))


def _seed_words(seed):
    return np.array(random.Random(seed).getstate()[1], np.uint32)


def _oracle(kw, s1, s2, seed, blosum=None, mtx=None):
    """(strings or None for the reference's IndexError, cost, score) of one pair under random.seed(seed)."""
    from oracle import core, transform
    a1, a2, smat, cmat, _, goc = transform.settings(dict(kw, seq_1=s1, seq_2=s2), blosum=blosum, mtx=mtx)
    r = core.align(a1, a2, cmat, goc, _seed_words(seed))
    score = transform.cost_to_score(r["cost"], len(a1), len(a2), transform.max_val(smat))
    return (r["strings"] if r["status"] == "ok" else None), r["cost"], score


def _check_pairs(ga, kw, pairs, seeds, want=None, **tables):
    """align_pairs(pairs, seeds) against the oracle (want: its results, when the caller has them already)."""
    P = len(pairs)
    eff = [seeds + k for k in range(P)] if isinstance(seeds, int) else list(seeds)
    if want is None:
        want = [_oracle(kw, s1, s2, s, **tables) for (s1, s2), s in zip(pairs, eff)]
    res = ga.GlobalAligner(max_seq_len_prod=None, **kw).align_pairs([p[0] for p in pairs], [p[1] for p in pairs],
                                                                    seeds=seeds)
    assert isinstance(res, ga.BatchAlignments)
    assert res.costs.dtype == np.int64 and res.scores.dtype == np.int64
    assert res.costs.shape == (P,) and res.scores.shape == (P,)
    assert len(res.seq_1_aligned) == len(res.middle_part) == len(res.seq_2_aligned) == P
    bad = [k for k in range(P)
           if (res.seq_1_aligned[k], res.middle_part[k], res.seq_2_aligned[k]) != want[k][0]
           or int(res.costs[k]) != want[k][1]]
    assert not bad, [(k, len(pairs[k][0]), len(pairs[k][1]), eff[k], int(res.costs[k]), want[k][1]) for k in bad[:8]]
    assert res.scores.tolist() == [w[2] for w in want]
    return res


def _edge_pairs(rng, count):
    """test_gpu_batch's corner shapes with the length-1 sides at 2 (m < 64, one / partial / several stripes), then
    mixed draws from EDGE_LENGTHS."""
    shapes = [(2, 2), (2, 513), (513, 2), (513, 513), (2, 300), (300, 3), (64, 64), (65, 129), (63, 257), (256, 255),
              (257, 64), (3, 65), (128, 128), (129, 127), (127, 513), (300, 300)]
    while len(shapes) < count:
        shapes.append((rng.choice(EDGE_LENGTHS), rng.choice(EDGE_LENGTHS)))
    return [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in shapes[:count]]


def test_stripe_edges_dna(ga):
    """Partial and multiple stripes, m < 64, two letters on either side; 8 of the pairs also against random.seed +
    the single call."""
    rng = random.Random(11)
    pairs = _edge_pairs(rng, 60)
    res = _check_pairs(ga, DNA, pairs, 1000)
    single = ga.GlobalAligner(max_seq_len_prod=None, **DNA)
    for k in (0, 1, 2, 3, 5, 9, 30, 59):
        random.seed(1000 + k)
        r = single.align(*pairs[k])
        assert r[:5] == res.result(k)[:5], k
        assert res.result(k).output is None
    assert res.gap_open_cost == 5 and res.gap_open_score == -5
    assert res.costing_mat["A"]["C"] == r.costing_mat["A"]["C"] and res.costing_mat["A"]["-"] == r.costing_mat["A"]["-"]


@pytest.mark.parametrize("o", [0, 6, 7, 126, 127, 300])
def test_gap_open_widths(ga, o):
    """One-, two- and four-byte traceback words, at the last gap-open cost of each width and the first of the next."""
    rng = random.Random(100 + o)
    _check_pairs(ga, dict(match_score=3, mismatch_score=-2, gap_open_score=-o, gap_extension_score=-1),
                 _edge_pairs(rng, 20), 5 * o)


def test_protein_blosum62(ga):
    """BLOSUM62, gap open 10: gH = 9 and gV = 10 (asymmetric), int8 profile, two-byte words; lengths 30-700."""
    rng = random.Random(62)
    pairs = [(splitmix_seq(rng.randint(30, 700), 2 * k + 1, "protein"), splitmix_seq(rng.randint(30, 700), 2 * k + 2, "protein"))
             for k in range(30)]
    _check_pairs(ga, dict(scoring_mat_name="BLOSUM62", gap_open_score=-10), pairs, 62, blosum=load_matrix("BLOSUM62"))


def test_matrix_file_int16_profile(ga, tmp_path):
    """A scoring matrix from a file whose sub' = sub - gV - gH needs the int16 profile (match: 0 - 200 - 200)."""
    letters = ["A", "C", "G", "T", "-"]
    scores = [[200 if x == y else -100 if "-" in (x, y) else -200 for y in letters] for x in letters]
    path = tmp_path / "wide.mtx"
    path.write_text("\n".join(["  ".join(letters)] + [letters[i] + " " + " ".join(str(v) for v in scores[i])
                                                      for i in range(len(letters))]) + "\n")
    from oracle import transform
    rng = random.Random(16)
    _check_pairs(ga, dict(scoring_mat_path=str(path), gap_open_score=-3), _edge_pairs(rng, 20), 16,
                 mtx=transform.read_mtx_rows(letters, scores))


def test_edge_column_and_scratch(ga):
    """Many stripes with the edge column in LDS and in HBM, and two pairs of different m sharing a wave's slices."""
    rng = random.Random(7)
    shapes = [(70, 5000), (5000, 70), (1100, 600), (1025, 1030), (40, 40)]
    _check_pairs(ga, DNA, [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in shapes], [7, 7, 2 ** 40, 0, 1])


def test_more_pairs_than_waves(ga):
    """6000 pairs of lengths 8-40: every resident wave takes several tickets and reuses its traceback slice, so a
    stale word of an earlier pair would show here; results come back in input order."""
    rng = random.Random(6000)
    pairs = [(_rand(rng, "ACGT", rng.randint(8, 40)), _rand(rng, "ACGT", rng.randint(8, 40))) for _ in range(6000)]
    _check_pairs(ga, DNA, pairs, 2 ** 32 - 3000)


def test_seeds(ga):
    rng = random.Random(77)
    pairs = [(_rand(rng, "ACGT", rng.randint(50, 300)), _rand(rng, "ACGT", rng.randint(50, 300))) for _ in range(40)]
    # a list with 0, equal seeds for different pairs, seeds >= 2^32
    seeds = [0, 5, 5, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1, 0] + [rng.randrange(2 ** 64) for _ in range(32)]
    want = [_oracle(DNA, s1, s2, s) for (s1, s2), s in zip(pairs, seeds)]
    res = _check_pairs(ga, DNA, pairs, seeds, want=want)
    # a base is the list base + k
    al = ga.GlobalAligner(**DNA)
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    by_base = al.align_pairs(a, b, seeds=2 ** 32 - 20)
    by_list = al.align_pairs(a, b, seeds=[2 ** 32 - 20 + k for k in range(40)])
    assert by_base[:3] == by_list[:3] and np.array_equal(by_base.costs, by_list.costs)
    # permuting the pairs together with their seeds permutes the results
    order = list(range(40))
    rng.shuffle(order)
    perm = al.align_pairs([a[k] for k in order], [b[k] for k in order], seeds=[seeds[k] for k in order])
    for field in range(3):
        assert perm[field] == [res[field][k] for k in order]
    assert np.array_equal(perm.costs, res.costs[order]) and np.array_equal(perm.scores, res.scores[order])
    # the seed matters: under seeds 0 and 1 at least one pair's strings differ
    zero, one = al.align_pairs(a, b, seeds=[0] * 40), al.align_pairs(a, b, seeds=[1] * 40)
    assert np.array_equal(zero.costs, one.costs)
    assert any(zero[f][k] != one[f][k] for f in range(3) for k in range(40))
    _check_pairs(ga, DNA, pairs[:10], [1] * 10)


def test_routing_gives_identical_results(ga, monkeypatch):
    """Mixed routes (GA_BATCH_ALIGN_MAX_CELLS=20000), every pair through the single-pair path (0) and the default:
    the same results, equal to the oracle's, in input order."""
    rng = random.Random(20000)
    pairs = [(_rand(rng, "ACGT", rng.randint(50, 600)), _rand(rng, "ACGT", rng.randint(50, 600))) for _ in range(24)]
    cells = [len(a) * len(b) for a, b in pairs]
    assert min(cells) <= 20000 < max(cells)
    want = [_oracle(DNA, s1, s2, 300 + k) for k, (s1, s2) in enumerate(pairs)]
    for limit in (20000, 0, None):
        if limit is not None:
            set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", limit)
        _check_pairs(ga, DNA, pairs, 300, want=want)
        monkeypatch.undo()


def test_table_threads_give_identical_results(ga, monkeypatch):
    rng = random.Random(8)
    pairs = [(_rand(rng, "ACGT", rng.randint(20, 120)), _rand(rng, "ACGT", rng.randint(20, 120))) for _ in range(300)]
    want = [_oracle(DNA, s1, s2, 40 + k) for k, (s1, s2) in enumerate(pairs)]
    for threads in (1, 8):
        set_knob(monkeypatch, "GA_BATCH_RNG_THREADS", threads)
        _check_pairs(ga, DNA, pairs, 40, want=want)
        monkeypatch.undo()


@pytest.mark.parametrize("kw", [dict(match_score=1, mismatch_score=-5, gap_extension_score=-1),
                                dict(mismatch_cost=9, gap_extension_cost=1)], ids=["scores", "costs"])
def test_one_letter_pairs_in_a_mixed_batch(ga, kw):
    """test_gpu_batch's mixed batch at gap open 60: pairs made of one letter keep their own max_cost (the sentinel
    leaks into the optimum) and their own score deltas.  Costs, scores and strings against random.seed + align.  The
    two pairs with a one-letter sequence raise the reference's IndexError under every seed at this gap open (the CPU
    oracle says so for 500 seeds), so a batch that returns cannot hold them: they are checked to raise and left out."""
    o = 60
    kw = dict(kw, **({"gap_open_score": -o} if "match_score" in kw else {"gap_open_cost": o}))
    rng = random.Random(o)
    pairs = [("ACGT", "ACGT"), ("AAA", "AA"), ("AAAAA", "AA"), ("aa", "AAAAAAA"), ("C", "CCCC"), ("TTTTTTTTT", "TT"),
             ("AAA", "CC"), ("ACG", "A"), ("G" * 70, "G" * 3), ("G" * 2, "G" * 130)]
    pairs += [(_rand(rng, "ACGT", rng.randint(2, 9)), _rand(rng, "ACGT", rng.randint(2, 9))) for _ in range(10)]
    single = ga.GlobalAligner(**kw)
    kept, want = [], []
    for k, (s1, s2) in enumerate(pairs):
        random.seed(900 + k)
        try:
            want.append(single.align(s1, s2))
            kept.append(k)
        except IndexError:
            assert min(len(s1), len(s2)) == 1
    assert len(kept) == 18
    res = ga.GlobalAligner(**kw).align_pairs([pairs[k][0] for k in kept], [pairs[k][1] for k in kept],
                                             seeds=[900 + k for k in kept])
    for q, k in enumerate(kept):
        assert res.result(q)[:5] == want[q][:5], (k, pairs[k])
    # and against the oracle under each pair's own matrices
    _check_pairs(ga, kw, [pairs[k] for k in kept], [900 + k for k in kept])


def test_length_one_pairs(ga):
    """A pair with a one-letter sequence inside a batch gives what random.seed(s) + align gives for its seed: the
    single call's result, or the reference's IndexError naming the pair.  One seed of each kind, found with the
    oracle, under settings where the walk of such a pair depends on the seed (DNA's gap open of 5 never raises, the
    one-letter batch's 60 always does)."""
    kw = dict(match_score=2, mismatch_score=-3, gap_open_score=-20, gap_extension_score=-1)
    rng = random.Random(1)
    others = [(_rand(rng, "ACGT", 30), _rand(rng, "ACGT", 33)), (_rand(rng, "ACGT", 5), _rand(rng, "ACGT", 4))]
    found = {}
    for short in (("A", "ACGT"), ("ACGT", "A")):
        for s in range(60):
            kind = _oracle(kw, short[0], short[1], s)[0] is not None
            found.setdefault((short, kind), s)
    good = [(short, s) for (short, kind), s in found.items() if kind]
    failing = [(short, s) for (short, kind), s in found.items() if not kind]
    assert len(good) == 2 and len(failing) == 2
    al = ga.GlobalAligner(**kw)
    for short, s in good:
        pairs, seeds = [others[0], short, others[1]], [3, s, 3]
        res = _check_pairs(ga, kw, pairs, seeds)
        random.seed(s)
        assert al.align(*short)[:5] == res.result(1)[:5]
    for short, s in failing:
        random.seed(s)
        with pytest.raises(IndexError):
            al.align(*short)
        with pytest.raises(IndexError) as e:
            al.align_pairs([others[0][0], others[1][0], short[0], short[0]], [others[0][1], others[1][1], short[1], short[1]],
                           seeds=[3, 3, s, s])
        assert str(e.value) == "pair 2: string index out of range"


def test_range_errors_come_before_index_errors(ga):
    """A pair out of the int32 range after a pair whose walk raises IndexError: the planner's error is raised."""
    kw = dict(mismatch_cost=10 ** 6, gap_open_cost=1, gap_extension_cost=1)
    rng = random.Random(10)
    large = (_rand(rng, "ACGT", 100), _rand(rng, "ACGT", 100))
    with pytest.raises(Exception) as batch:
        ga.GlobalAligner(**kw).align_pairs(["A", large[0]], ["ACGT", large[1]], seeds=0)
    assert not isinstance(batch.value, IndexError)
    assert "pair 1" in str(batch.value) and "int32 score range" in str(batch.value)


def test_state_between_calls(ga):
    """A find_global_alignment call before and after a batch returns what it returns without it, with the same random
    state; align_pairs leaves random alone; score_pairs on the same pairs returns the same costs."""
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
        al = ga.GlobalAligner(**DNA)
        res = _check_pairs(ga, DNA, first, 17)
        scored = al.score_pairs([p[0] for p in first], [p[1] for p in first])
        assert np.array_equal(scored.costs, res.costs) and np.array_equal(scored.scores, res.scores)
        _check_pairs(ga, DNA, second, [2 ** 64 - 1 - k for k in range(9)])
        assert random.getstate() == before

    assert two_calls(batches) == two_calls(lambda: None)
