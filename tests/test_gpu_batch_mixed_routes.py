"""Kernel-route chunks and large-route pairs in one call of sample_alignments, count_alignments, alignments_by_rank
and match_support.  The four calls share one stored-words fill stage and one large-route stage, and
both stage their work list in bt_items and their slices in bs_words: a large-route pair's one-item lists follow the
chunks' in the same buffers.  The results must not depend on the route."""
import random

import numpy as np
import pytest

from tests.conftest import set_knob

pytestmark = pytest.mark.gpu

# With GA_BATCH_ALIGN_MAX_CELLS=4096 the first four stay on the kernel route and the last two take the large route;
# (70, 130) has two stripes.  The four kernel pairs' slices are 512, 640, 832 and 960 u32 words at one-byte words, so
# GA_BATCH_SAMPLE_CHUNK_WORDS=1500 cuts them into several chunks.
SHAPES = [(30, 30), (40, 41), (50, 51), (60, 61), (80, 81), (70, 130)]
KNOBS = {"GA_BATCH_ALIGN_MAX_CELLS": 4096, "GA_BATCH_SAMPLE_CHUNK_WORDS": 1500}
CALLS = ["sample", "count", "rank", "support"]
OWN_BUFFERS = {"sample": {"bs_words", "bs_tb", "bs_witems", "bs_ticket"},
               "count": {"bc_out", "bc_ticket"},
               "rank": {"br_table", "br_toff", "br_out", "br_ranks", "br_items", "br_ticket"},
               "support": {"bm_table", "bm_toff", "bm_ooff", "bm_out", "bm_count", "bm_ticket"}}


@pytest.fixture(scope="module")
def ga():
    import globalign_amd
    from globalign_amd import _native
    assert _native.device_count() >= 1
    return globalign_amd


def _engine():
    from globalign_amd import _native
    return _native.default_engine(0)


@pytest.fixture(scope="module")
def pairs():
    rng = random.Random(1500)
    return [("".join(rng.choice("ACGT") for _ in range(m)), "".join(rng.choice("ACGT") for _ in range(n)))
            for m, n in SHAPES]


def _run(ga, call, pairs):
    """The call on the pairs and its info; for sample_alignments a pair with a one-letter sequence follows them, which
    takes the per-sample loop."""
    al = ga.GlobalAligner(max_seq_len_prod=None)
    A, B = [p[0] for p in pairs], [p[1] for p in pairs]
    if call == "sample":
        return al.sample_alignments(A + ["G"], B + ["ACGTTGCA"], samples=3, seeds=77), _engine().batch_sample_info()
    if call == "count":
        return al.count_alignments(A, B), _engine().batch_count_info()
    if call == "rank":
        return al.alignments_by_rank(A, B, [[0, 1, 2, 3]] * len(A)), _engine().batch_rank_info()
    return al.match_support(A, B), _engine().batch_support_info()


def _same(x, y):
    if isinstance(x, np.ndarray):
        return isinstance(y, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
    if isinstance(x, (list, tuple)):
        return type(x) is type(y) and len(x) == len(y) and all(_same(p, q) for p, q in zip(x, y))
    return x == y


def _assert_same(got, want):
    assert type(got) is type(want)
    for name in want._fields:
        assert _same(getattr(got, name), getattr(want, name)), name


def _assert_mixed(call, info):
    """Four kernel pairs in more than one chunk and two large-route pairs."""
    if call == "sample":
        assert (info["filled_pairs"], info["single_fill_pairs"], info["looped_pairs"]) == (4, 2, 1), info
        assert info["fill_launches"] - info["single_fill_pairs"] > 1, info  # (every chunk and large-route pair: a fill)
        assert info["walk_items"] == 3 * 6, info
    else:
        assert (info["kernel_pairs"], info["single_fill_pairs"]) == (4, 2) and info["fill_chunks"] > 1, info
        assert info["fill_launches"] == info["fill_chunks"] + 2, info


def _assert_default(call, info):
    if call == "sample":
        assert (info["filled_pairs"], info["single_fill_pairs"], info["looped_pairs"], info["fill_launches"]) == (6, 0, 1, 1)
    else:
        assert (info["kernel_pairs"], info["single_fill_pairs"], info["fill_chunks"]) == (6, 0, 1), info


@pytest.mark.parametrize("call", CALLS)
def test_mixed_routes_equal_the_default_route(ga, pairs, monkeypatch, call):
    base, info = _run(ga, call, pairs)
    _assert_default(call, info)
    if call == "rank":
        assert (base.counts >= 4).all() and all(len(s) == 4 for s in base.seq_1_aligned)
    for name, value in KNOBS.items():
        set_knob(monkeypatch, name, value)
    mixed, info = _run(ga, call, pairs)
    _assert_mixed(call, info)
    _assert_same(mixed, base)
    # The same context again (contexts are cached by their knobs): its chunks now follow the large route's one-item
    # work list and slice in bt_items / bs_words.  This run shows that such stale lists are harmless.
    again, info = _run(ga, call, pairs)
    _assert_mixed(call, info)
    _assert_same(again, base)
    # and with the knobs removed, which is a fresh context: the default route still gives the same
    monkeypatch.undo()
    plain, info = _run(ga, call, pairs)
    _assert_default(call, info)
    _assert_same(plain, base)


@pytest.mark.parametrize("call", CALLS)
def test_guards(ga, pairs, monkeypatch, call):
    """The mixed routes with guard bands on every device buffer: no kernel stores out of range (no GA_E_GUARD), and the
    call's own buffers are among the guarded ones."""
    base, _ = _run(ga, call, pairs)
    set_knob(monkeypatch, "GA_GUARD_BYTES", 4096)
    for name, value in KNOBS.items():
        set_knob(monkeypatch, name, value)
    mixed, info = _run(ga, call, pairs)
    _assert_mixed(call, info)
    _assert_same(mixed, base)
    rep = _engine().guard_report()
    assert rep["guard_bytes"] == 4096 and rep["violations"] == []
    listed = {b["name"] for b in rep["buffers"] if b["guarded"]}
    assert OWN_BUFFERS[call] | {"bt_items", "bt_out"} <= listed
