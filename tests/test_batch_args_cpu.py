"""The batched calls' argument layer (globalign_amd._native.batch_arrays / batch_outputs): one normaliser for
Engine.batch_costs, batch_align and batch_sample.  Every malformed input raises the ValueError the three methods always
raised, in their order; a well-formed input comes back in the engine's dtypes with hand-computed offsets and buffer
sizes.  No GPU: the module imports without a device."""
import numpy as np
import pytest

from globalign_amd import _native

E_SHAPES = "pair_a and pair_b must be 1-d and of equal length, seq_off 1-d and non-empty"
E_END_COSTS = "seq_off must end at len(codes)"
E_END_STRINGS = "seq_off must end at len(codes), and chars must hold one byte per code"
E_SEEDS_PAIR = "seeds must have one entry per pair"
E_SEEDS_SAMPLE = "seeds must have one entry per sample"
E_SAMPLE_OFF = "sample_off must have one entry per pair and one more, start at 0 and not decrease"
E_INDEX = "sequence index out of range"
E_PMC = "pair_max_cost must have one entry per pair"


def good():
    """Three sequences of 3, 2 and 4 letters; the pairs (0, 1), (2, 0), (1, 1); 2, 0 and 3 samples."""
    return dict(codes=[0, 1, 2, 3, 0, 1, 2, 3, 0], seq_off=[0, 3, 5, 9], pair_a=[0, 2, 1], pair_b=[1, 0, 1],
                pair_max_cost=[5, 6, 7], chars=list(b"ACGTACGTA"), seeds=[10, 11, 12], sample_off=[0, 2, 2, 5])


def call(kind, **changes):
    a = good()
    a.update(changes)
    if kind == "costs":
        return _native.batch_arrays(a["codes"], a["seq_off"], a["pair_a"], a["pair_b"], a["pair_max_cost"])
    if kind == "align":
        return _native.batch_arrays(a["codes"], a["seq_off"], a["pair_a"], a["pair_b"], a["pair_max_cost"], a["chars"],
                                    a["seeds"])
    if "seeds" not in changes:
        a["seeds"] = [20, 21, 22, 23, 24]
    return _native.batch_arrays(a["codes"], a["seq_off"], a["pair_a"], a["pair_b"], a["pair_max_cost"], a["chars"],
                                a["seeds"], a["sample_off"])


def refused(kind, text, **changes):
    with pytest.raises(ValueError) as e:
        call(kind, **changes)
    assert str(e.value) == text


@pytest.mark.parametrize("kind", ["costs", "align", "sample"])
def test_shapes_and_ends(kind):
    refused(kind, E_SHAPES, pair_a=[0, 2])                          # unequal pair arrays
    refused(kind, E_SHAPES, pair_a=[[0, 2, 1]], pair_b=[[1, 0, 1]])  # 2-d pair arrays
    refused(kind, E_SHAPES, seq_off=[[0, 3, 5, 9]])                  # 2-d seq_off
    refused(kind, E_SHAPES, seq_off=[])
    end = E_END_COSTS if kind == "costs" else E_END_STRINGS
    refused(kind, end, seq_off=[0, 3, 5, 8])
    refused(kind, end, codes=[0, 1, 2])
    # a wrong pair_max_cost: 2 entries, and 2-d
    refused(kind, E_PMC, pair_max_cost=[5, 6])
    refused(kind, E_PMC, pair_max_cost=[[5, 6, 7]])
    # the shapes come first, then the ends, pair_max_cost last
    refused(kind, E_SHAPES, pair_a=[0], seq_off=[0, 3, 5, 8], pair_max_cost=[1])
    refused(kind, end, seq_off=[0, 3, 5, 8], pair_max_cost=[1])


@pytest.mark.parametrize("kind", ["align", "sample"])
def test_strings_calls(kind):
    refused(kind, E_END_STRINGS, chars=list(b"ACGTACGT"))   # chars of another size
    refused(kind, E_END_STRINGS, chars=list(b"ACGTACGTAC"))
    refused(kind, E_INDEX, pair_a=[0, 3, 1])                # an index out of range, either side and sign
    refused(kind, E_INDEX, pair_b=[1, 0, -1])
    seeds_text = E_SEEDS_PAIR if kind == "align" else E_SEEDS_SAMPLE
    refused(kind, seeds_text, seeds=[1, 2])                 # seeds of the wrong length
    refused(kind, seeds_text, seeds=[[1, 2, 3, 4, 5]])
    # chars before seeds, seeds before the indices, the indices before pair_max_cost
    refused(kind, E_END_STRINGS, chars=[65], seeds=[1], pair_a=[0, 3, 1])
    refused(kind, seeds_text, seeds=[1], pair_a=[0, 3, 1], pair_max_cost=[1])
    refused(kind, E_INDEX, pair_a=[0, 3, 1], pair_max_cost=[1])


def test_sample_off():
    refused("sample", E_SAMPLE_OFF, sample_off=[0, 2, 5])        # one entry short
    refused("sample", E_SAMPLE_OFF, sample_off=[1, 2, 2, 5])     # does not start at 0
    refused("sample", E_SAMPLE_OFF, sample_off=[0, 3, 2, 5])     # decreases
    refused("sample", E_SAMPLE_OFF, sample_off=[[0, 2, 2, 5]])
    # sample_off before the seeds, which are counted by its last entry
    refused("sample", E_SAMPLE_OFF, sample_off=[0, 2, 5], seeds=[1])
    refused("sample", E_SEEDS_SAMPLE, sample_off=[0, 2, 2, 6])
    refused("sample", E_SEEDS_SAMPLE, seeds=[10, 11, 12])        # per pair, not per sample


def test_costs_gains_no_check():
    """batch_costs never looked at the sequence indices (the engine's planner does): it still does not."""
    b = call("costs", pair_a=[0, 7, 1])
    assert b.pair_a.tolist() == [0, 7, 1] and b.chars is None and b.seeds is None and b.sample_off is None


def test_well_formed():
    for kind in ("costs", "align", "sample"):
        b = call(kind)
        want = [("codes", np.uint8, 9), ("seq_off", np.int64, 4), ("pair_a", np.int32, 3), ("pair_b", np.int32, 3),
                ("pair_max_cost", np.int32, 3)]
        if kind != "costs":
            want += [("chars", np.uint8, 9), ("seeds", np.uint64, 3 if kind == "align" else 5)]
        if kind == "sample":
            want += [("sample_off", np.int64, 4)]
        for name, dtype, size in want:
            x = getattr(b, name)
            assert x.dtype == dtype and x.shape == (size,) and x.flags["C_CONTIGUOUS"], (kind, name)
        assert b.P == 3 and b.S == {"costs": 0, "align": 3, "sample": 5}[kind]
        assert b.pmc is not None and b.pmc[0] == 5 and b.pmc[2] == 7
    assert call("costs", pair_max_cost=None).pmc is None
    assert call("align").chars.tobytes() == b"ACGTACGTA"
    # a strided input is made contiguous
    b = call("align", pair_a=np.array([0, 9, 2, 9, 1, 9])[::2])
    assert b.pair_a.tolist() == [0, 2, 1] and b.pair_a.flags["C_CONTIGUOUS"]


def test_offsets_and_buffers():
    # pair lengths 3 + 2, 4 + 3, 2 + 2; a slot holds m + n + 1 bytes
    offsets, bufs, costs, lengths, status = _native.batch_outputs(call("align"))
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 6, 14, 19]
    assert len(bufs) == 3 and all(x.dtype == np.uint8 and x.shape == (19,) for x in bufs)
    assert bufs[0] is not bufs[1] and bufs[1] is not bufs[2]
    assert (costs.dtype, costs.shape) == (np.int64, (3,)) and (lengths.dtype, lengths.shape) == (np.int64, (3,))
    assert (status.dtype, status.shape) == (np.int32, (3,)) and not costs.any() and not lengths.any() and not status.any()
    # samples 2, 0, 3: two slots of 6 bytes, none of 8, three of 5
    offsets, bufs, costs, lengths, status = _native.batch_outputs(call("sample"))
    assert offsets.tolist() == [0, 6, 12, 17, 22, 27]
    assert all(x.shape == (27,) for x in bufs) and costs.shape == (3,) and lengths.shape == (5,) and status.shape == (5,)
    # no sample at all: one-byte buffers and one-entry arrays, so that every pointer is valid
    offsets, bufs, costs, lengths, status = _native.batch_outputs(call("sample", sample_off=[0, 0, 0, 0], seeds=[]))
    assert offsets.tolist() == [0] and all(x.shape == (1,) for x in bufs)
    assert costs.shape == (3,) and lengths.shape == (1,) and status.shape == (1,)
