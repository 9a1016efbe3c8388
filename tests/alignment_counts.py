"""The expected number of co-optimal alignments of a pair, in pure Python: what GlobalAligner.count_alignments must
return (tests/test_batch_count_host.py pins this helper against the reference's own traceback, tests/
test_gpu_batch_count.py compares the GPU with it).

The reference's traceback (dp_array_backward, globaligner.py:395-593) is a walk on the states (i, j, L), L the level
of the last move.  At (i, j, L) it ranks the cell's triple plus costs_to_add (:487-514) and random.choice picks among
the entries of rank 0; the set of those entries is S_L(i, j).  The alignments it can return are the paths from
(m, n, 0) to row 0 or column 0, where the tail is forced:

    T0 = N(i-1, j-1, 0)   T1 = N(i, j-1, 1)   T2 = N(i-1, j, 2)
    N(i, j, L) = sum of T_k over k in S_L(i, j);   N = 1 where i == 0 or j == 0;   count = N(m, n, 0)

Everything here is deterministic and imports without pytest.
"""
import random

import numpy as np

from oracle import core

# the pinned tiny pairs (everyday DNA settings) with their counts, and the seed range over which the reference returns
# every one of a pair's co-optimal alignments: verified once against the oracle's align (the outcome is deterministic)
PINNED_SEEDS = range(400)
PINNED = [
    ("AGGCG", "TCGATGC", 1), ("CGTCACG", "ACCGGCTG", 2), ("ACAT", "CGCCCCGC", 2), ("TCC", "GG", 3),
    ("TTTATC", "CG", 4), ("ATAAC", "CGAT", 5), ("AGTTT", "TATT", 7), ("CAACTCA", "GCTTCG", 10),
]


def filled_array(seq_1, seq_2, cmat, o):
    """The reference's filled dp array of the pair as an int64 array (m + 1, n + 1, 3), from the oracle's fill."""
    tab = core.Tables(cmat)
    a, b = tab.codes(seq_1), tab.codes(seq_2)
    m, n = len(a), len(b)
    big = (tab.max_cost + 1) * max(m, n)
    row0, col0 = core.boundary(tab, a, b, o, big)
    dp = np.zeros((m + 1, n + 1, 3), np.int64)
    dp[0, :, :] = row0.reshape(n + 1, 3)
    dp[:, 0, :] = col0.reshape(m + 1, 3)
    return core.fill_full(tab, a, b, o, dp)


def rank_sets(dp, o):
    """Per interior cell (i, j) -> [i - 1, j - 1] and entering level L, the entries of rank 0 as bits (bit k: level
    k), S_L at bits 3L .. 3L + 2.  costs_to_add as in dp_array_backward: the same cost on all three at level 0, the
    gap open cost on the two entries that open or switch a gap at levels 1 and 2 (the term common to all three does
    not change a rank and is left out)."""
    cells = dp[1:, 1:, :]
    out = np.zeros(cells.shape[:2], dtype=np.int64)
    for L, add in enumerate(((0, 0, 0), (o, 0, o), (o, o, 0))):
        v = cells + np.array(add, dtype=np.int64)
        rank0 = v == v.min(axis=2, keepdims=True)
        out |= (rank0[:, :, 0] * 1 + rank0[:, :, 1] * 2 + rank0[:, :, 2] * 4) << (3 * L)
    return out


def count_from_sets(sets):
    """N(m, n, 0) of an (m, n) array of packed sets, carried twice: as Python ints (exact) and as Python floats with
    the terms added in the order T0, T1, T2 (an unselected term adds 0.0, which is exact).  -> (int, float)"""
    m, n = sets.shape
    # row i - 1 of N(., ., 0) and N(., ., 2), ints and floats; column 0 and row 0 hold 1
    i0, f0 = [1] * (n + 1), [1.0] * (n + 1)
    i2, f2 = [1] * (n + 1), [1.0] * (n + 1)
    for row in sets.tolist():
        ai, af = i0[0], f0[0]      # T0 = N(i-1, j-1, 0)
        bi, bf = 1, 1.0            # T1 = N(i, j-1, 1)
        for j in range(1, n + 1):
            s = row[j - 1]
            ci, cf = i2[j], f2[j]  # T2 = N(i-1, j, 2)
            n0i = (ai if s & 1 else 0) + (bi if s & 2 else 0) + (ci if s & 4 else 0)
            n0f = ((af if s & 1 else 0.0) + (bf if s & 2 else 0.0)) + (cf if s & 4 else 0.0)
            n1i = (ai if s & 8 else 0) + (bi if s & 16 else 0) + (ci if s & 32 else 0)
            n1f = ((af if s & 8 else 0.0) + (bf if s & 16 else 0.0)) + (cf if s & 32 else 0.0)
            i2[j] = (ai if s & 64 else 0) + (bi if s & 128 else 0) + (ci if s & 256 else 0)
            f2[j] = ((af if s & 64 else 0.0) + (bf if s & 128 else 0.0)) + (cf if s & 256 else 0.0)
            ai, af = i0[j], f0[j]
            i0[j], f0[j] = n0i, n0f
            bi, bf = n1i, n1f
    return i0[n], f0[n]


def expected_count(seq_1, seq_2, cmat, o):
    """(int count, float count) of the pair under the costing dict and gap open cost; min(m, n) >= 2."""
    assert min(len(seq_1), len(seq_2)) >= 2
    return count_from_sets(rank_sets(filled_array(seq_1, seq_2, cmat, o), o))


def costs_of(seq_1="ACGT", seq_2="ACGT", blosum=None, **settings):
    """(costing dict, gap open cost) of the settings (none: the everyday DNA ones) over the pair's letters, by the
    oracle's transform; blosum: the named matrix's scores (tests.conftest.load_matrix) when the settings name one."""
    from oracle import transform
    good = transform.settings(dict(settings, seq_1=seq_1, seq_2=seq_2), blosum=blosum)
    return good[3], good[5]


def reference_distinct(seq_1, seq_2, cmat, o, seeds):
    """The number of different (seq_1_aligned, seq_2_aligned) the reference's traceback returns over random.seed(s)
    for s in seeds, by the oracle's align."""
    seen = set()
    for s in seeds:
        words = np.array(random.Random(s).getstate()[1], dtype=np.uint32)
        got = core.align(seq_1, seq_2, cmat, o, words)
        assert got["status"] == "ok"
        seen.add((got["strings"][0], got["strings"][2]))
    return len(seen)
