"""The expected match support of a pair, in pure Python: what GlobalAligner.match_support must return
(tests/test_batch_support_host.py pins this helper against a brute-force tally and against the reference's own
traceback, tests/test_gpu_batch_support.py compares the GPU with it).  Builds on tests/alignment_ranks.py, whose Ranked
has the state DAG (i, j, L), the sets S_L(i, j) and the exact backward path counts N(i, j, L).

F(i, j, L) counts the walk prefixes from (m, n, 0) to a state:

    F(m, n, .) = (1, 0, 0)
    F(i, j, 0) = A_0(i+1, j+1)   F(i, j, 1) = A_1(i, j+1)   F(i, j, 2) = A_2(i+1, j)        (0 outside the matrix)
    A_k(i, j) = (f_0 + f_1) + f_2,  f_L = F(i, j, L) if k in S_L(i, j) else 0
    support(i, j) = A_0(i, j) * N(i-1, j-1, 0)

Everything here is deterministic and imports without pytest.
"""
import numpy as np


def _plane0_floats(rows, n):
    """N(i, j, 0) in Python floats, the terms added in the order T0, T1, T2 (tests/alignment_counts.py
    count_from_sets): a list of m + 1 rows of n + 1."""
    out = [[1.0] * (n + 1)]
    f2 = [1.0] * (n + 1)
    for row in rows:
        prev, cur = out[-1], [1.0] * (n + 1)
        bf = 1.0
        for j in range(1, n + 1):
            s = row[j - 1]
            af, cf = prev[j - 1], f2[j]
            cur[j] = ((af if s & 1 else 0.0) + (bf if s & 2 else 0.0)) + (cf if s & 4 else 0.0)
            bf, f2[j] = (((af if s & 8 else 0.0) + (bf if s & 16 else 0.0)) + (cf if s & 32 else 0.0),
                         ((af if s & 64 else 0.0) + (bf if s & 128 else 0.0)) + (cf if s & 256 else 0.0))
        out.append(cur)
    return out


def support_model(R):
    """The pair's supports by the recurrence, carried twice: as exact Python ints and as Python floats in the order
    above.  R: a tests.alignment_ranks.Ranked.  -> (ints: m lists of n ints, floats: numpy float64 (m, n), the float
    count)"""
    m, n, rows = R.m, R.n, R.rows
    Ni, Nf = R.N[0], _plane0_floats(rows, n)
    ints = [[0] * n for _ in range(m)]
    floats = np.zeros((m, n), dtype=np.float64)
    # A_0 and A_2 of row i + 1, columns 1 .. n + 1: row m + 1 and column n + 1 hold 0
    a0i, a2i, a0f, a2f = [0] * (n + 2), [0] * (n + 2), [0.0] * (n + 2), [0.0] * (n + 2)
    for i in range(m, 0, -1):
        row, out_i, out_f = rows[i - 1], ints[i - 1], floats[i - 1]
        pni, pnf = Ni[i - 1], Nf[i - 1]
        di, df, ri, rf = 0, 0.0, 0, 0.0     # A_0(i + 1, j + 1) and A_1(i, j + 1)
        for j in range(n, 0, -1):
            s = row[j - 1]
            f0i, f1i, f2i, f0f, f1f, f2f = di, ri, a2i[j], df, rf, a2f[j]
            if i == m and j == n:
                f0i, f1i, f2i, f0f, f1f, f2f = 1, 0, 0, 1.0, 0.0, 0.0
            x0i = (f0i if s & 1 else 0) + (f1i if s & 8 else 0) + (f2i if s & 64 else 0)
            x0f = ((f0f if s & 1 else 0.0) + (f1f if s & 8 else 0.0)) + (f2f if s & 64 else 0.0)
            ri = (f0i if s & 2 else 0) + (f1i if s & 16 else 0) + (f2i if s & 128 else 0)
            rf = ((f0f if s & 2 else 0.0) + (f1f if s & 16 else 0.0)) + (f2f if s & 128 else 0.0)
            di, df = a0i[j], a0f[j]
            a0i[j], a0f[j] = x0i, x0f
            a2i[j] = (f0i if s & 4 else 0) + (f1i if s & 32 else 0) + (f2i if s & 256 else 0)
            a2f[j] = ((f0f if s & 4 else 0.0) + (f1f if s & 32 else 0.0)) + (f2f if s & 256 else 0.0)
            out_i[j - 1] = x0i * pni[j - 1]
            out_f[j - 1] = x0f * pnf[j - 1]
    return ints, floats, Nf[m][n]


def tally_levels(R, all_levels):
    """Letter-letter columns tallied over level sequences from (m, n): -> m lists of n ints."""
    out = [[0] * R.n for _ in range(R.m)]
    for levels in all_levels:
        i, j = R.m, R.n
        for lv in levels:
            if lv == 0:
                out[i - 1][j - 1] += 1
            i -= lv != 1
            j -= lv != 2
    return out


def brute_force(R):
    """The supports by walking every path of the pair's DAG (small pairs only)."""
    return tally_levels(R, R.all_levels())


def tally_strings(m, n, alignments):
    """Letter-letter columns tallied over alignments given as (seq_1_aligned, seq_2_aligned): -> m lists of n ints."""
    out = [[0] * n for _ in range(m)]
    for a, b in alignments:
        i = j = 0
        for x, y in zip(a, b):
            if x != "-" and y != "-":
                out[i][j] += 1
            i += x != "-"
            j += y != "-"
        assert (i, j) == (m, n)
    return out
