"""GPU tests of the device route of align_pairs' tie-break tables (batch_rng_kernel through ga_debug_pair_tables and
ga_batch_align_ex).  The oracle for a table is CPython itself: random.Random(seed)'s 18 choices per dispatch, packed as
the engine packs them; the oracle for alignments is test_gpu_batch_align's CPU oracle."""
import random

import numpy as np
import pytest

from tests.conftest import load_matrix, set_knob, splitmix_seq
from tests.test_gpu_batch_align import DNA, _check_pairs, _edge_pairs, _oracle, _rand

pytestmark = pytest.mark.gpu

SIZES = (3, 2, 2, 2, 3, 2, 2, 2, 3, 3, 2, 2, 2, 3, 2, 2, 2, 3)
EDGE_SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1]
GUARD = 0xA5A5A5A5


@pytest.fixture(scope="module")
def ga():
    import globalign_amd
    from globalign_amd import _native
    assert _native.device_count() >= 1
    return globalign_amd


def _engine():
    from globalign_amd import _native
    return _native.default_engine(0)


def cpython_table(seed, steps):
    """The entries of `steps` dispatches under random.seed(seed), from random.choice itself."""
    r = random.Random(seed)
    ranges = [range(s) for s in SIZES]
    out = np.zeros(steps, dtype=np.uint32)
    for d in range(steps):
        draws = [r.choice(x) for x in ranges]
        e = 0
        for half in (0, 1):
            q = draws[9 * half:]
            for S, level in enumerate((0, 1, q[1], 2, 2 * q[2], 1 + q[3], q[0]), start=1):
                e |= level << (2 * S + 1 + 14 * half)
        out[d] = e
    return out


def test_tables_against_cpython_by_both_routes(ga, monkeypatch):
    """One launch of 15 seeds x 9 step counts: 19 / 20 / 21 and 39 / 40 straddle block boundaries (a 624-word block
    holds 19.5 dispatches on average), 700 and 5000 take many blocks (the item limit raised so that the device makes
    them too)."""
    set_knob(monkeypatch, "GA_BATCH_RNG_DEVICE_MAX_STEPS", 8192)
    rng = random.Random(2024)
    seeds = EDGE_SEEDS + [rng.randrange(2 ** 64) if k % 2 else rng.randrange(2 ** 32) for k in range(8)]
    step_counts = [1, 4, 19, 20, 21, 39, 40, 700, 5000]
    want = {s: cpython_table(s, max(step_counts)) for s in seeds}
    items = [(s, n) for s in seeds for n in step_counts]
    eng = _engine()
    for route in ("device", "host"):
        tab, off, status = eng.debug_pair_tables([s for s, _ in items], [n for _, n in items], rng_tables=route)
        assert status.tolist() == [0] * len(items), route
        bad = [(s, n) for k, (s, n) in enumerate(items) if not np.array_equal(tab[off[k]:off[k + 1]], want[s][:n])]
        assert not bad, (route, bad[:5])
        info = eng.batch_align_info()
        if route == "device":
            assert (info["device_items"], info["host_items"], info["fell_back"]) == (len(items), 0, False)
            assert info["generator_blocks"] == (len(items) + 3) // 4
        else:
            assert (info["device_items"], info["host_items"], info["generator_blocks"]) == (0, len(items), 0)


def test_many_items_stay_inside_their_ranges(ga):
    """5000 items of 4-80 dispatches in one launch: the device's tables equal the host's bit for bit, and the guard
    words the debug entry lays between the items' ranges on the device are intact (status 2 otherwise)."""
    rng = random.Random(5000)
    seeds = [rng.randrange(2 ** 64) if k % 3 else k for k in range(5000)]
    steps = [rng.randint(4, 80) for _ in range(5000)]
    eng = _engine()
    dev, off, status = eng.debug_pair_tables(seeds, steps, rng_tables="device")
    assert eng.batch_align_info()["device_items"] == 5000 and eng.batch_align_info()["generator_blocks"] == 1250
    assert not status.any(), np.flatnonzero(status)[:8]
    host, off_h, status_h = eng.debug_pair_tables(seeds, steps, rng_tables="host")
    assert not status_h.any() and np.array_equal(off, off_h) and int(off[-1]) == sum(steps)
    assert not (dev == GUARD).any()
    assert np.array_equal(dev, host), np.flatnonzero(dev != host)[:8]


def test_debug_entry_honours_limit_and_cap(ga, monkeypatch):
    """An item over GA_BATCH_RNG_DEVICE_MAX_STEPS is built on the host, at the limit on the device; under
    GA_BATCH_RNG_WORD_CAP=24 a long item stops with status 1, its entries up to the stop right and the rest unwritten,
    while an item that needs fewer words than its cap's blocks hold completes."""
    set_knob(monkeypatch, "GA_BATCH_RNG_DEVICE_MAX_STEPS", 300)
    eng = _engine()
    want = cpython_table(9, 2000)
    tab, off, status = eng.debug_pair_tables([9, 9, 9], [299, 300, 301], rng_tables="device")
    info = eng.batch_align_info()
    assert (info["device_items"], info["host_items"], info["generator_blocks"]) == (2, 1, 1)
    assert status.tolist() == [0, 0, 0]
    for k, n in enumerate((299, 300, 301)):
        assert np.array_equal(tab[off[k]:off[k + 1]], want[:n])
    monkeypatch.undo()
    set_knob(monkeypatch, "GA_BATCH_RNG_WORD_CAP", 24)
    set_knob(monkeypatch, "GA_BATCH_RNG_DEVICE_MAX_STEPS", 2000)
    eng = _engine()
    tab, off, status = eng.debug_pair_tables([9, 9], [2000, 4], rng_tables="device")
    assert status.tolist() == [1, 0]
    long_item = tab[:2000]
    written = int(np.argmax(long_item == GUARD))
    # the cap's blocks hold ceil((24 * 2000 + 624) / 624) * 624 = 48672 words; a dispatch takes 18 at the least and
    # 32 on average, so the stop lies between
    assert 48672 // 70 <= written < 2000 and (long_item[written:] == GUARD).all()
    assert np.array_equal(long_item[:written], want[:written])
    assert np.array_equal(tab[off[1]:off[2]], want[:4])


def _pairs_and_lists(pairs):
    return [p[0] for p in pairs], [p[1] for p in pairs]


def test_align_pairs_device_against_the_oracle(ga, monkeypatch):
    """The 60 edge-shape DNA pairs under seed base 1000 and 10 BLOSUM62 pairs of 30-700 letters with tables="device":
    strings, costs and scores against the CPU oracle, the global random state untouched, every kernel pair's table
    made by the device and no fallback (the item limit raised to 8192: the longest pair has 1400 dispatches)."""
    set_knob(monkeypatch, "GA_BATCH_RNG_DEVICE_MAX_STEPS", 8192)
    before = random.getstate()
    rng = random.Random(11)
    pairs = _edge_pairs(rng, 60)
    want = [_oracle(DNA, s1, s2, 1000 + k) for k, (s1, s2) in enumerate(pairs)]
    a, b = _pairs_and_lists(pairs)
    res = ga.GlobalAligner(max_seq_len_prod=None, **DNA).align_pairs(a, b, seeds=1000, tables="device")
    info = _engine().batch_align_info()
    assert (info["device_items"], info["host_items"], info["fell_back"]) == (60, 0, False)
    assert info["generator_blocks"] == 15
    for k in range(60):
        assert (res.seq_1_aligned[k], res.middle_part[k], res.seq_2_aligned[k]) == want[k][0], k
    assert res.costs.tolist() == [w[1] for w in want] and res.scores.tolist() == [w[2] for w in want]

    rng = random.Random(62)
    kw = dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)
    prot = [(splitmix_seq(rng.randint(30, 700), 2 * k + 1, "protein"), splitmix_seq(rng.randint(30, 700), 2 * k + 2, "protein"))
            for k in range(10)]
    want = [_oracle(kw, s1, s2, 62 + k, blosum=load_matrix("BLOSUM62")) for k, (s1, s2) in enumerate(prot)]
    a, b = _pairs_and_lists(prot)
    res = ga.GlobalAligner(max_seq_len_prod=None, **kw).align_pairs(a, b, seeds=62, tables="device")
    info = _engine().batch_align_info()
    assert (info["device_items"], info["host_items"], info["fell_back"]) == (10, 0, False)
    for k in range(10):
        assert (res.seq_1_aligned[k], res.middle_part[k], res.seq_2_aligned[k]) == want[k][0], k
    assert res.costs.tolist() == [w[1] for w in want] and res.scores.tolist() == [w[2] for w in want]
    assert random.getstate() == before


def _same(x, y):
    return x[:3] == y[:3] and np.array_equal(x.costs, y.costs) and np.array_equal(x.scores, y.scores)


def test_mixed_routes(ga, monkeypatch):
    """GA_BATCH_RNG_DEVICE_MAX_STEPS=300 over pairs of 50-600 letters: tables from both routes in one launch; with
    GA_BATCH_ALIGN_MAX_CELLS=20000 some pairs also take the single-pair path.  The host route's results, and the info
    counts the lengths predict."""
    rng = random.Random(300)
    pairs = [(_rand(rng, "ACGT", rng.randint(50, 600)), _rand(rng, "ACGT", rng.randint(50, 600))) for _ in range(24)]
    a, b = _pairs_and_lists(pairs)
    al = ga.GlobalAligner(**DNA)
    host = al.align_pairs(a, b, seeds=300)
    for max_cells in (None, 20000):
        set_knob(monkeypatch, "GA_BATCH_RNG_DEVICE_MAX_STEPS", 300)
        if max_cells is not None:
            set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", max_cells)
        kernel = [(len(x), len(y)) for x, y in pairs if max_cells is None or len(x) * len(y) <= max_cells]
        n_dev = sum(m + n <= 300 for m, n in kernel)
        assert 0 < n_dev < len(kernel) and (max_cells is None or len(kernel) < len(pairs))
        res = al.align_pairs(a, b, seeds=300, tables="device")
        info = _engine().batch_align_info()
        assert (info["device_items"], info["host_items"], info["fell_back"]) == (n_dev, len(kernel) - n_dev, False)
        assert info["generator_blocks"] == (n_dev + 3) // 4
        assert _same(res, host)
        monkeypatch.undo()


def test_fallback_at_the_word_cap(ga, monkeypatch):
    """GA_BATCH_RNG_WORD_CAP=24 on 20 pairs of 400-1000 dispatches (they take 32 words each on average): the
    generator stops, the info says so, and the results are the host route's."""
    rng = random.Random(24)
    pairs = [(_rand(rng, "ACGT", rng.randint(200, 500)), _rand(rng, "ACGT", rng.randint(200, 500))) for _ in range(20)]
    a, b = _pairs_and_lists(pairs)
    al = ga.GlobalAligner(**DNA)
    host = al.align_pairs(a, b, seeds=24)
    set_knob(monkeypatch, "GA_BATCH_RNG_WORD_CAP", 24)
    res = al.align_pairs(a, b, seeds=24, tables="device")
    info = _engine().batch_align_info()
    assert info["fell_back"] and info["device_items"] == 20 and info["generator_blocks"] == 5
    assert _same(res, host)
    # and a later call on the same context is a device call again
    monkeypatch.undo()
    res = al.align_pairs(a, b, seeds=24, tables="device")
    assert not _engine().batch_align_info()["fell_back"] and _same(res, host)


def test_single_pair_path_launches_no_generator(ga, monkeypatch):
    rng = random.Random(0)
    pairs = [(_rand(rng, "ACGT", rng.randint(20, 200)), _rand(rng, "ACGT", rng.randint(20, 200))) for _ in range(6)]
    a, b = _pairs_and_lists(pairs)
    al = ga.GlobalAligner(**DNA)
    host = al.align_pairs(a, b, seeds=5)
    set_knob(monkeypatch, "GA_BATCH_ALIGN_MAX_CELLS", 0)
    res = al.align_pairs(a, b, seeds=5, tables="device")
    info = _engine().batch_align_info()
    assert info == dict(device_items=0, host_items=0, fell_back=False, generator_blocks=0)
    assert _same(res, host)


def test_context_default_and_bad_options(ga, monkeypatch):
    """GA_BATCH_RNG=device makes the device route the context's default (align_pairs' "host" passes no route); bad
    option values are refused when the context is created."""
    from globalign_amd import _native
    rng = random.Random(1)
    pairs = [(_rand(rng, "ACGT", 40), _rand(rng, "ACGT", 50)) for _ in range(5)]
    _check_pairs(ga, DNA, pairs, 77)
    assert _engine().batch_align_info()["device_items"] == 0
    set_knob(monkeypatch, "GA_BATCH_RNG", "device")
    _check_pairs(ga, DNA, pairs, 77)
    assert _engine().batch_align_info()["device_items"] == 5
    monkeypatch.undo()
    for name, value in (("GA_BATCH_RNG", "gpu"), ("GA_BATCH_RNG_DEVICE_MAX_STEPS", -1),
                        ("GA_BATCH_RNG_DEVICE_MAX_STEPS", 2 ** 21), ("GA_BATCH_RNG_WORD_CAP", 0)):
        with pytest.raises(ValueError):
            _native.Engine(0, options={name: value})
