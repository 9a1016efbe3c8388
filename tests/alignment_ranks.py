"""The expected co-optimal alignments of a pair by rank, in pure Python: what GlobalAligner.alignments_by_rank must
return (tests/test_batch_rank_host.py pins this helper against the reference's own traceback, tests/
test_gpu_batch_rank.py compares the GPU with it).  Builds on tests/alignment_counts.py, which has the state DAG
(i, j, L), the sets S_L(i, j) and the count recurrence.

The alignments of a pair are the paths from (m, n, 0) to row 0 or column 0.  They are ordered by their level sequence
as the traceback emits it (from the alignment's last column backwards), lexicographically with level 0 (diagonal) <
level 1 (left, gap in seq_1) < level 2 (up, gap in seq_2).  The walk for rank r goes, at a state, through the selected
k of S_L in the order 0, 1, 2: if r < T_k it takes move k, else r -= T_k.  All counts here are exact Python ints.

Everything here is deterministic and imports without pytest.
"""
from tests import alignment_counts as ac

CAP = 2 ** 64 - 1   # the engine's counts saturate here; ranks below min(count, CAP) are exact all the same


class Ranked:
    """A pair's state DAG with its exact path counts: count, levels(r), strings(r), all_levels()."""

    def __init__(self, seq_1, seq_2, sets):
        self.seq_1, self.seq_2 = seq_1, seq_2
        self.m, self.n = sets.shape
        assert (self.m, self.n) == (len(seq_1), len(seq_2))
        self.rows = sets.tolist()
        n = self.n
        # N[L][i][j] = N(i, j, L); row 0 and column 0 hold 1
        N0, N1, N2 = [[1] * (n + 1)], [[1] * (n + 1)], [[1] * (n + 1)]
        for row in self.rows:
            p0, p2 = N0[-1], N2[-1]
            r0, r1, r2 = [1] * (n + 1), [1] * (n + 1), [1] * (n + 1)
            for j in range(1, n + 1):
                s = row[j - 1]
                t0, t1, t2 = p0[j - 1], r1[j - 1], p2[j]
                r0[j] = (t0 if s & 1 else 0) + (t1 if s & 2 else 0) + (t2 if s & 4 else 0)
                r1[j] = (t0 if s & 8 else 0) + (t1 if s & 16 else 0) + (t2 if s & 32 else 0)
                r2[j] = (t0 if s & 64 else 0) + (t1 if s & 128 else 0) + (t2 if s & 256 else 0)
            N0.append(r0), N1.append(r1), N2.append(r2)
        self.N = (N0, N1, N2)
        self.count = N0[self.m][n]

    def levels(self, r):
        """The level sequence of the alignment of rank r, 0 <= r < count."""
        assert 0 <= r < self.count
        i, j, L, out = self.m, self.n, 0, []
        while i > 0 and j > 0:
            S = (self.rows[i - 1][j - 1] >> (3 * L)) & 7
            for k in (0, 1, 2):
                if not (S >> k) & 1:
                    continue
                pi, pj = i - (k != 1), j - (k != 2)
                t = self.N[k][pi][pj]
                if r < t:
                    break
                r -= t
            else:
                raise AssertionError("the rank is not below the state's count")
            out.append(k)
            i, j, L = pi, pj, k
        return out

    def strings(self, r):
        """(seq_1_aligned, middle_part, seq_2_aligned) of the alignment of rank r."""
        return levels_to_strings(self.levels(r), self.seq_1, self.seq_2)

    def all_levels(self):
        """Every path's level sequence in depth-first order, moves tried in the order 0, 1, 2 (small pairs only)."""
        out = []

        def go(i, j, L, cur):
            if i == 0 or j == 0:
                out.append(list(cur))
                return
            S = (self.rows[i - 1][j - 1] >> (3 * L)) & 7
            for k in (0, 1, 2):
                if (S >> k) & 1:
                    cur.append(k)
                    go(i - (k != 1), j - (k != 2), k, cur)
                    cur.pop()

        go(self.m, self.n, 0, [])
        return out


def levels_to_strings(levels, seq_1, seq_2):
    """A level sequence from (m, n) to the three lines: `|` match, `*` mismatch, space at gaps; the forced tail after
    row 0 (the rest of seq_2 under gaps) or column 0 (the rest of seq_1 over gaps); then the reversal."""
    i, j = len(seq_1), len(seq_2)
    a, mid, b = [], [], []
    for lv in levels:
        assert i >= 1 and j >= 1
        ca, cb = seq_1[i - 1], seq_2[j - 1]
        a.append("-" if lv == 1 else ca)
        mid.append(" " if lv else ("|" if ca == cb else "*"))
        b.append("-" if lv == 2 else cb)
        i -= lv != 1
        j -= lv != 2
    assert i == 0 or j == 0
    for jj in range(j, 0, -1):
        a.append("-"), mid.append(" "), b.append(seq_2[jj - 1])
    for ii in range(i, 0, -1):
        a.append(seq_1[ii - 1]), mid.append(" "), b.append("-")
    return "".join(reversed(a)), "".join(reversed(mid)), "".join(reversed(b))


def ranked(seq_1, seq_2, cmat, o):
    """The pair's Ranked under the costing dict and gap open cost; min(m, n) >= 2; the sequences upper-cased."""
    assert min(len(seq_1), len(seq_2)) >= 2
    return Ranked(seq_1, seq_2, ac.rank_sets(ac.filled_array(seq_1, seq_2, cmat, o), o))


def alignment_cost(strings, cmat, o):
    """The cost of an alignment from its three lines: every column's entry of the costing dict, plus the gap open cost
    where a gap run starts in either sequence."""
    a, _, b = strings
    cost, prev = 0, None
    for x, y in zip(a, b):
        cost += cmat[x][y]
        kind = 1 if x == "-" else 2 if y == "-" else 0
        if kind and kind != prev:
            cost += o
        prev = kind
    return cost
