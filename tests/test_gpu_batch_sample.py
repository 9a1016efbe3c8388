"""GPU parity of GlobalAligner.sample_alignments (ga_batch_sample: batch_words_kernel fills a pair once,
batch_walks_kernel walks it once per sample): sample t of pair k against the CPU oracle's alignment from the state
random.seed(s_kt) leaves -- strings, cost, score --, as tests/test_gpu_batch_align.py checks align_pairs."""
import random

import numpy as np
import pytest

from tests.conftest import load_matrix, set_knob, splitmix_seq

pytestmark = pytest.mark.gpu

DNA = dict(match_score=2, mismatch_score=-3, gap_open_score=-5, gap_extension_score=-1)
EDGE_SHAPES = [(2, 2), (2, 513), (513, 2), (513, 513), (2, 300), (300, 3), (64, 64), (65, 129), (63, 257), (256, 255),
               (257, 64), (3, 65), (128, 128), (129, 127), (127, 513), (300, 300)]
NEW_BUFFERS = {"bs_words", "bs_tb", "bs_witems", "bs_ticket"}


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


def _seed_words(seed):
    return np.array(random.Random(seed).getstate()[1], np.uint32)


def _oracle(kw, s1, s2, seed, blosum=None, mtx=None):
    """(strings or None for the reference's IndexError, cost, score) of one pair under random.seed(seed)."""
    from oracle import core, transform
    a1, a2, smat, cmat, _, goc = transform.settings(dict(kw, seq_1=s1, seq_2=s2), blosum=blosum, mtx=mtx)
    r = core.align(a1, a2, cmat, goc, _seed_words(seed))
    score = transform.cost_to_score(r["cost"], len(a1), len(a2), transform.max_val(smat))
    return (r["strings"] if r["status"] == "ok" else None), r["cost"], score


def _flat_seeds(counts, seeds):
    if isinstance(seeds, int):
        out, f = [], seeds
        for c in counts:
            out.append(list(range(f, f + c)))
            f += c
        return out
    return [list(s) for s in seeds]


def _want(kw, pairs, counts, seeds, **tables):
    return [[_oracle(kw, s1, s2, s, **tables) for s in own] for (s1, s2), own in zip(pairs, _flat_seeds(counts, seeds))]


def _check_samples(ga, kw, pairs, counts, seeds, want=None, tables="host", **oracle_tables):
    """sample_alignments(pairs, counts, seeds) against the oracle (want: its results, when the caller has them)."""
    P = len(pairs)
    if want is None:
        want = _want(kw, pairs, counts, seeds, **oracle_tables)
    res = ga.GlobalAligner(max_seq_len_prod=None, **kw).sample_alignments(
        [p[0] for p in pairs], [p[1] for p in pairs], samples=counts, seeds=seeds, tables=tables)
    assert isinstance(res, ga.BatchSamples)
    assert res.costs.dtype == np.int64 and res.scores.dtype == np.int64
    assert res.costs.shape == (P,) and res.scores.shape == (P,)
    assert [len(x) for x in res.seq_1_aligned] == counts == [len(x) for x in res.middle_part]
    assert [len(x) for x in res.seq_2_aligned] == counts
    assert [s.tolist() for s in res.seeds] == _flat_seeds(counts, seeds)
    bad = [(k, t) for k in range(P) for t in range(counts[k])
           if (res.seq_1_aligned[k][t], res.middle_part[k][t], res.seq_2_aligned[k][t]) != want[k][t][0]
           or int(res.costs[k]) != want[k][t][1] or int(res.scores[k]) != want[k][t][2]]
    assert not bad, [(k, t, len(pairs[k][0]), len(pairs[k][1]), int(res.costs[k]), want[k][t][1]) for k, t in bad[:8]]
    return res


def _same(x, y):
    return x[:3] == y[:3] and np.array_equal(x.costs, y.costs) and np.array_equal(x.scores, y.scores)


@pytest.fixture(scope="module")
def edge_batch():
    """The 16 corner shapes of test_gpu_batch_align's _edge_pairs x 4 samples, DNA, with the oracle's results."""
    rng = random.Random(11)
    pairs = [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in EDGE_SHAPES]
    counts = [4] * len(pairs)
    return pairs, counts, 1000, _want(DNA, pairs, counts, 1000)


LARGE_SHAPES = [(65, 129), (300, 257), (513, 513), (70, 1500)]


@pytest.fixture(scope="module")
def large_batch():
    rng = random.Random(4096)
    pairs = [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in LARGE_SHAPES]
    counts = [4] * len(pairs)
    return pairs, counts, 77, _want(DNA, pairs, counts, 77)


def test_stripe_edges_dna(ga, edge_batch):
    """Partial and multiple stripes, m < 64, two letters on either side; a few samples also against random.seed +
    the single call."""
    pairs, counts, base, want = edge_batch
    res = _check_samples(ga, DNA, pairs, counts, base, want=want)
    info = _engine().batch_sample_info()
    assert info["filled_pairs"] == 16 and info["walk_items"] == 64 and info["fill_launches"] == 1
    assert info["walk_launches"] == 1 and info["single_fill_pairs"] == 0 and info["looped_pairs"] == 0
    assert info["host_items"] == 64 and info["device_items"] == 0
    single = ga.GlobalAligner(max_seq_len_prod=None, **DNA)
    for k, t in ((0, 0), (3, 3), (9, 1), (15, 2)):
        random.seed(base + 4 * k + t)
        r = single.align(*pairs[k])
        assert r[:5] == res.result(k, t)[:5], (k, t)
        assert res.result(k, t).output is None
    assert res.gap_open_cost == 5 and res.gap_open_score == -5


@pytest.mark.parametrize("o", [6, 7, 127])
def test_gap_open_widths(ga, o):
    """One-, two- and four-byte traceback words: 8 pairs x 3 samples."""
    rng = random.Random(100 + o)
    shapes = EDGE_SHAPES[3:4] + EDGE_SHAPES[7:12] + [(40, 90), (17, 5)]
    pairs = [(_rand(rng, "ACGT", m), _rand(rng, "ACGT", n)) for m, n in shapes]
    _check_samples(ga, dict(match_score=3, mismatch_score=-2, gap_open_score=-o, gap_extension_score=-1), pairs,
                   [3] * 8, 5 * o)


def test_protein_blosum62(ga):
    """BLOSUM62, gap open 10: gH = 9 and gV = 10 (asymmetric), int8 profile, two-byte words; lengths 30-300."""
    rng = random.Random(62)
    pairs = [(splitmix_seq(rng.randint(30, 300), 2 * k + 1, "protein"), splitmix_seq(rng.randint(30, 300), 2 * k + 2, "protein"))
             for k in range(6)]
    _check_samples(ga, dict(scoring_mat_name="BLOSUM62", gap_open_score=-10), pairs, [3] * 6, 62,
                   blosum=load_matrix("BLOSUM62"))


def test_equals_align_pairs_and_leaves_random_alone(ga):
    """One batch with different counts and nested seeds against align_pairs on the flattened, repeated lists, byte
    for byte; the process's random state is untouched."""
    rng = random.Random(5)
    pairs = [(_rand(rng, "ACGT", rng.randint(20, 400)), _rand(rng, "ACGT", rng.randint(20, 400))) for _ in range(9)]
    counts = [1, 5, 2, 3, 1, 4, 2, 6, 3]
    seeds = [[rng.randrange(2 ** 64) for _ in range(c)] for c in counts]
    seeds[1][0] = seeds[1][1] = 0           # equal seeds give equal samples
    seeds[7][5] = 2 ** 64 - 1
    al = ga.GlobalAligner(**DNA)
    random.seed(123)
    before = random.getstate()
    res = al.sample_alignments([p[0] for p in pairs], [p[1] for p in pairs], seeds=seeds)
    assert random.getstate() == before
    flat_a = [pairs[k][0] for k in range(9) for _ in range(counts[k])]
    flat_b = [pairs[k][1] for k in range(9) for _ in range(counts[k])]
    flat = al.align_pairs(flat_a, flat_b, seeds=[s for own in seeds for s in own])
    f = 0
    for k in range(9):
        for t in range(counts[k]):
            assert res.result(k, t) == flat.result(f), (k, t)
            f += 1
    assert res.seq_1_aligned[1][0] == res.seq_1_aligned[1][1] and res.middle_part[1][0] == res.middle_part[1][1]
    assert [s.tolist() for s in res.seeds] == seeds
    # a base numbers the samples flat in pair order
    by_base = al.sample_alignments([p[0] for p in pairs], [p[1] for p in pairs], samples=counts, seeds=2 ** 32 - 10)
    flat = al.align_pairs(flat_a, flat_b, seeds=2 ** 32 - 10)
    assert [x for own in by_base.seq_1_aligned for x in own] == flat.seq_1_aligned
    assert [x for own in by_base.middle_part for x in own] == flat.middle_part
    assert [x for own in by_base.seq_2_aligned for x in own] == flat.seq_2_aligned
    assert random.getstate() == before


def test_more_walk_items_than_waves(ga):
    """3 pairs of 8-40 letters x 2200 samples: 6600 walk items on at most 2048 waves, so every wave takes several
    tickets."""
    rng = random.Random(6600)
    pairs = [(_rand(rng, "ACGT", rng.randint(8, 40)), _rand(rng, "ACGT", rng.randint(8, 40))) for _ in range(3)]
    _check_samples(ga, DNA, pairs, [2200] * 3, 2 ** 32 - 3000)
    info = _engine().batch_sample_info()
    assert info["filled_pairs"] == 3 and info["walk_items"] == 6600 and info["walk_launches"] == 1


def test_distinct_samples(ga):
    """The issue's 300 x 257 pair at seeds 100 .. 163: 64 distinct alignments, all at cost 735, and distinct(0) agrees
    with the oracle's."""
    rng = random.Random(5)
    a = "".join(rng.choice("ACGT") for _ in range(300))
    b = "".join(rng.choice("ACGT") for _ in range(257))
    want = _want(DNA, [(a, b)], [64], 100)
    assert len({w[0] for w in want[0]}) == 64 and {w[1] for w in want[0]} == {735}
    res = _check_samples(ga, DNA, [(a, b)], [64], 100, want=want)
    assert int(res.costs[0]) == 735
    assert res.distinct(0) == [(w[0], 1) for w in want[0]]


def test_forced_chunking(ga, monkeypatch):
    """Tiny caps on the fill chunk's words and a walk launch's table entries: the same results from several fill and
    walk launches, every pair still filled once."""
    rng = random.Random(55)
    pairs = [(_rand(rng, "ACGT", 40 + 10 * k), _rand(rng, "ACGT", 41 + 10 * k)) for k in range(5)]
    want = _want(DNA, pairs, [5] * 5, 9)
    _check_samples(ga, DNA, pairs, [5] * 5, 9, want=want)
    info = _engine().batch_sample_info()
    assert info["fill_launches"] == 1 and info["walk_launches"] == 1 and info["filled_pairs"] == 5
    # (a pair of 80 x 81 has a slice of 20 rows of u32s x 128 columns = 2560 words, and 161 table entries a walk)
    set_knob(monkeypatch, "GA_BATCH_SAMPLE_CHUNK_WORDS", 5200)
    set_knob(monkeypatch, "GA_BATCH_SAMPLE_WALK_ENTRIES", 500)
    _check_samples(ga, DNA, pairs, [5] * 5, 9, want=want)
    info = _engine().batch_sample_info()
    assert info["fill_launches"] > 1 and info["walk_launches"] > info["fill_launches"]
    assert info["filled_pairs"] == 5 and info["walk_items"] == 25 and info["single_fill_pairs"] == 0
    assert info["looped_pairs"] == 0


def test_device_tables(ga, edge_batch):
    """tables="device" equals "host" on the edge batch; the info counts the items the generator made (m + n <= 1024,
    its default limit) and those the host made beside it."""
    pairs, counts, base, want = edge_batch
    _check_samples(ga, DNA, pairs, counts, base, want=want, tables="device")
    info = _engine().batch_sample_info()
    n_dev = 4 * sum(m + n <= 1024 for m, n in EDGE_SHAPES)
    assert 0 < n_dev < 64
    assert info["device_items"] == n_dev and info["host_items"] == 64 - n_dev and info["walk_items"] == 64


def test_fallback_at_the_word_cap(ga, monkeypatch):
    """GA_BATCH_RNG_WORD_CAP=24 on walks of 400-1000 dispatches (they take 32 words each on average): the generator
    stops, the walk launch runs again with host tables -- the fill does not --, and the results are the oracle's."""
    rng = random.Random(24)
    pairs = [(_rand(rng, "ACGT", rng.randint(200, 500)), _rand(rng, "ACGT", rng.randint(200, 500))) for _ in range(4)]
    want = _want(DNA, pairs, [3] * 4, 24)
    set_knob(monkeypatch, "GA_BATCH_RNG_WORD_CAP", 24)
    _check_samples(ga, DNA, pairs, [3] * 4, 24, want=want, tables="device")
    info = _engine().batch_sample_info()
    assert info["fill_launches"] == 1 and info["walk_launches"] == 2 and info["filled_pairs"] == 4
    assert info["device_items"] == 12 and info["host_items"] == 12 and info["walk_items"] == 12
    monkeypatch.undo()
    _check_samples(ga, DNA, pairs, [3] * 4, 24, want=want, tables="device")
    info = _engine().batch_sample_info()
    assert info["walk_launches"] == 1 and info["device_items"] == 12 and info["host_items"] == 0


def test_large_route_at_small_size(ga, large_batch, monkeypatch):
    """GA_BATCH_ALIGN_MAX_CELLS=4096 sends every pair to the single-pair fill with stored words, once each; their
    samples walk those words in the fill's own layout."""
    pairs, counts, base, want = large_batch
    set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", 4096)
    _check_samples(ga, DNA, pairs, counts, base, want=want)
    info = _engine().batch_sample_info()
    assert info["single_fill_pairs"] == 4 and info["filled_pairs"] == 0 and info["looped_pairs"] == 0
    assert info["walk_items"] == 16 and info["walk_launches"] == 4
    # word widths on that route
    for o in (7, 127):
        kw = dict(match_score=3, mismatch_score=-2, gap_open_score=-o, gap_extension_score=-1)
        _check_samples(ga, kw, pairs[:2], [2, 2], 3 * o)
        assert _engine().batch_sample_info()["single_fill_pairs"] == 2
    monkeypatch.undo()
    # the same batch at the defaults stays on the kernel route and gives the same results
    _check_samples(ga, DNA, pairs, counts, base, want=want)
    assert _engine().batch_sample_info()["filled_pairs"] == 4


def test_large_route_with_both_table_routes(ga, large_batch, monkeypatch):
    """The single-pair fills' walk launches under tables="device" with the generator's limit at 600 dispatches: the
    pairs of 194 and 557 have their tables from the device, those of 1026 and 1570 from the host."""
    pairs, counts, base, want = large_batch
    set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", 4096)
    set_knob(monkeypatch, "GA_BATCH_RNG_DEVICE_MAX_STEPS", 600)
    assert min(m + n for m, n in LARGE_SHAPES) < 600 < max(m + n for m, n in LARGE_SHAPES)
    _check_samples(ga, DNA, pairs, counts, base, want=want, tables="device")
    info = _engine().batch_sample_info()
    n_dev = sum(c for (m, n), c in zip(LARGE_SHAPES, counts) if m + n <= 600)
    assert info["single_fill_pairs"] == 4 and info["filled_pairs"] == 0 and info["walk_items"] == 16
    assert n_dev == 8 and info["device_items"] == n_dev and info["host_items"] == 16 - n_dev


def test_large_route_fallback_at_the_word_cap(ga, large_batch, monkeypatch):
    """GA_BATCH_RNG_WORD_CAP=24 with every pair's tables on the device (walks of 194-1570 dispatches take 32 words each
    on average): each single-pair fill's walk launch runs again with host tables, the fills do not."""
    pairs, counts, base, want = large_batch
    set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", 4096)
    set_knob(monkeypatch, "GA_BATCH_RNG_DEVICE_MAX_STEPS", 2000)
    _check_samples(ga, DNA, pairs, counts, base, want=want, tables="device")
    uncapped = _engine().batch_sample_info()
    assert uncapped["single_fill_pairs"] == 4 and uncapped["device_items"] == 16 and uncapped["host_items"] == 0
    set_knob(monkeypatch, "GA_BATCH_RNG_WORD_CAP", 24)
    _check_samples(ga, DNA, pairs, counts, base, want=want, tables="device")
    info = _engine().batch_sample_info()
    assert info["walk_launches"] == 2 * uncapped["walk_launches"] == 8
    assert info["fill_launches"] == uncapped["fill_launches"] and info["single_fill_pairs"] == 4
    assert info["device_items"] == 16 and info["host_items"] == 16 and info["walk_items"] == 16


def test_large_route_at_the_defaults(ga):
    """One 2000 x 1500 pair (3e6 cells, above the default limit of 2^20) x 8 samples."""
    pair = (splitmix_seq(2000, 1, "dna"), splitmix_seq(1500, 2, "dna"))
    _check_samples(ga, DNA, [pair], [8], 2000)
    info = _engine().batch_sample_info()
    assert info["single_fill_pairs"] == 1 and info["filled_pairs"] == 0 and info["looped_pairs"] == 0
    assert info["walk_items"] == 8


def test_one_letter_pairs(ga):
    """Pairs with a one-letter sequence are looped sample by sample through the single-pair path and equal the oracle;
    under test_gpu_batch_align.test_length_one_pairs's settings (the walk of such a pair depends on the seed) a sample
    that raises the reference's IndexError makes the call raise it for the lowest such pair."""
    kw = dict(match_score=2, mismatch_score=-3, gap_open_score=-20, gap_extension_score=-1)
    rng = random.Random(1)
    other = (_rand(rng, "ACGT", 30), _rand(rng, "ACGT", 33))
    shorts = [("A", "ACGT"), ("ACGT", "A")]
    good = {s: [x for x in range(60) if _oracle(kw, s[0], s[1], x)[0] is not None] for s in shorts}
    bad = {s: [x for x in range(60) if _oracle(kw, s[0], s[1], x)[0] is None] for s in shorts}
    assert all(len(good[s]) >= 3 and bad[s] for s in shorts)
    pairs = [other, shorts[0], shorts[1]]
    seeds = [[3, 4, 5], good[shorts[0]][:3], good[shorts[1]][:3]]
    _check_samples(ga, kw, pairs, [3, 3, 3], seeds)
    info = _engine().batch_sample_info()
    assert info["looped_pairs"] == 2 and info["filled_pairs"] == 1 and info["walk_items"] == 3
    al = ga.GlobalAligner(**kw)
    with pytest.raises(IndexError) as e:
        al.sample_alignments([other[0], "A", "ACGT"], [other[1], "ACGT", "A"],
                             seeds=[[3], [good[shorts[0]][0], bad[shorts[0]][0]], [bad[shorts[1]][0]]])
    assert str(e.value) == "pair 1: string index out of range"
    # DNA's gap open of 5 never raises: a mixed batch with one-letter pairs
    _check_samples(ga, DNA, [("C", "CCCC"), other, ("ACG", "A")], [2, 2, 2], 900)


@pytest.mark.parametrize("which", ["edge", "large"])
def test_guards(ga, edge_batch, large_batch, monkeypatch, which):
    """The edge batch and the large-route batch with guard bands on every device buffer: no kernel stores out of
    range, and the call's own buffers are among the guarded ones."""
    set_knob(monkeypatch, "GA_GUARD_BYTES", 4096)
    if which == "edge":
        pairs, counts, base, want = edge_batch
    else:
        pairs, counts, base, want = large_batch
        set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", 4096)
    _check_samples(ga, DNA, pairs, counts, base, want=want)
    info = _engine().batch_sample_info()
    assert (info["filled_pairs"], info["single_fill_pairs"]) == ((16, 0) if which == "edge" else (0, 4))
    rep = _engine().guard_report()
    assert rep["guard_bytes"] == 4096 and rep["violations"] == []
    listed = {b["name"] for b in rep["buffers"] if b["guarded"]}
    assert NEW_BUFFERS - {"bs_tb"} <= listed and ("bs_tb" in listed) == (which == "edge")
    assert "fb.tb" in listed or which == "edge"
