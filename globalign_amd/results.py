"""Alignment result type and the cost -> score conversion.

Mirror of the reference's src/globalign/conclude.py: AlignmentResults
(:7-151, same ten fields, same printout), final_cost_to_score (:154-177),
final_score_to_cost (:179-202) and prettify_mat (:252-310).
"""
import math
from pathlib import Path
from typing import NamedTuple


def final_cost_to_score(cost, m, n, max_score, delta_d=None, delta_i=None):
    """score = n * floor(b/2) + m * ceil(b/2) - cost."""
    dd = math.floor(max_score / 2) if delta_d is None else delta_d
    di = math.ceil(max_score / 2) if delta_i is None else delta_i
    return n * dd + m * di - cost


def final_score_to_cost(score, m, n, max_score, delta_d=None, delta_i=None):
    dd = math.floor(max_score / 2) if delta_d is None else delta_d
    di = math.ceil(max_score / 2) if delta_i is None else delta_i
    return -score + n * dd + m * di


def print_nested_list_aligned(nested_list):
    """Print a list of equal-length rows with every column right-aligned to its widest cell + 1
    (conclude.py:204-249)."""
    widths = [max(len(str(row[j])) for row in nested_list) for j in range(len(nested_list[0]))]
    print("".join("".join(f"{str(c):>{w + 1}}" for c, w in zip(row, widths)) + "\n" for row in nested_list))


def prettify_mat(mat):
    """Right-aligned text table of a nested-dict matrix with row and column headers."""
    try:
        cols = list(list(mat.values())[0].keys())
    except Exception:
        print("mat does not appear to represent a matrix as a nested dictionary.")
        raise
    widths = [max([len(str(c))] + [len(str(mat[r][c])) for r in mat.keys()]) for c in cols]
    head_w = max(len(str(c)) for c in cols)
    parts = [" " * (head_w + 1)]
    parts += [f"{str(c):>{w + 1}}" for c, w in zip(cols, widths)]
    for r in mat.keys():
        parts.append("\n")
        parts.append(f"{str(r):<{head_w + 1}}")
        parts += [f"{str(mat[r][c]):>{w + 1}}" for c, w in zip(cols, widths)]
    return "".join(parts)


class BatchScores(NamedTuple):
    """Costs and scores of many pairs (GlobalAligner.score_pairs / score_matrix): numpy int64 arrays, shape (P,) for
    a pair list and (N1, N2) for a matrix, with the settings every pair was scored under."""
    costs: "numpy.ndarray"
    scores: "numpy.ndarray"
    scoring_mat: dict
    costing_mat: dict
    gap_open_score: int
    gap_open_cost: int


class AlignmentResults(NamedTuple):
    seq_1_aligned: str
    middle_part: str
    seq_2_aligned: str
    cost: int
    score: int
    scoring_mat: dict
    costing_mat: dict
    gap_open_score: int
    gap_open_cost: int
    output: Path

    def _generate_alignment_printout(self, desc_1="seq_1", desc_2="seq_2", chars_per_line=70):
        L = len(self.middle_part)
        blocks = math.ceil(L / chars_per_line)
        yield desc_1
        yield "\n"
        yield desc_2
        lo = 0
        hi = L if blocks == 1 else chars_per_line
        for _ in range(blocks):
            yield "\n\n"
            yield self.seq_1_aligned[lo:hi]
            yield "\n"
            yield self.middle_part[lo:hi]
            yield "\n"
            yield self.seq_2_aligned[lo:hi]
            lo, hi = hi, hi + chars_per_line
        yield "\n\n"
        yield f"score: {self.score}\n"
        yield f"cost: {self.cost}\n"
        yield "###########################################\n# Settings\n###########################################\n"
        yield "scoring_mat:\n"
        yield prettify_mat(self.scoring_mat)
        yield f"\n\ngap_open_score: {self.gap_open_score}\n"
        yield "\ncosting_mat:\n"
        yield prettify_mat(self.costing_mat)
        yield f"\n\ngap_open_cost: {self.gap_open_cost}\n"

    def __str__(self, desc_1="seq_1", desc_2="seq_2", chars_per_line=70):
        return "".join(self._generate_alignment_printout(desc_1=desc_1, desc_2=desc_2, chars_per_line=chars_per_line))

    def print(self, desc_1="seq_1", desc_2="seq_2", chars_per_line=70):
        print(self.__str__(desc_1=desc_1, desc_2=desc_2, chars_per_line=chars_per_line))

    def write(self, file=None, desc_1="seq_1", desc_2="seq_2", chars_per_line=70):
        """Write to `file`, else to self.output, else (or file == "stdout") to stdout."""
        if (file is None and self.output is None) or file == "stdout":
            self.print(desc_1=desc_1, desc_2=desc_2, chars_per_line=chars_per_line)
            return None
        target = self.output if file is None else file
        text = self.__str__(desc_1=desc_1, desc_2=desc_2, chars_per_line=chars_per_line)
        with open(file=target, mode="w+") as fh:
            fh.write(text)
        return None

    def cigar(self):
        """Extended CIGAR of the alignment (=: match, X: mismatch, D: gap in seq_2, I: gap in seq_1).

        Not part of the reference; derived from the middle line and the gap characters."""
        ops = []
        for a, mid, b in zip(self.seq_1_aligned, self.middle_part, self.seq_2_aligned):
            ops.append("=" if mid == "|" else "X" if mid == "*" else ("I" if a == "-" else "D"))
        out, k = [], 0
        while k < len(ops):
            q = k
            while q < len(ops) and ops[q] == ops[k]:
                q += 1
            out.append(f"{q - k}{ops[k]}")
            k = q
        return "".join(out)


class BatchAlignments(NamedTuple):
    """Alignments of many pairs (GlobalAligner.align_pairs): per pair the three strings, in lists, and the cost and
    score, in numpy int64 arrays of shape (P,), with the settings every pair was aligned under.  The matrices are the
    batch's -- for match / mismatch settings they span the letters of the whole batch --, not those the single call
    builds over one pair's own letters; every entry a pair reads is the same in both."""
    seq_1_aligned: list
    middle_part: list
    seq_2_aligned: list
    costs: "numpy.ndarray"
    scores: "numpy.ndarray"
    scoring_mat: dict
    costing_mat: dict
    gap_open_score: int
    gap_open_cost: int

    def result(self, k):
        """Pair k as an AlignmentResults (output=None), with the batch's matrices."""
        return AlignmentResults(self.seq_1_aligned[k], self.middle_part[k], self.seq_2_aligned[k], int(self.costs[k]),
                                int(self.scores[k]), self.scoring_mat, self.costing_mat, self.gap_open_score,
                                self.gap_open_cost, None)


class BatchSamples(NamedTuple):
    """Many seeded alignments of every pair (GlobalAligner.sample_alignments): per pair a list with one string per
    sample, for each of the three lines; the pair's cost and score, which do not depend on the seed, in numpy int64
    arrays of shape (P,); per pair the uint64 array of its samples' seeds; and the settings, as BatchAlignments
    reports them."""
    seq_1_aligned: list
    middle_part: list
    seq_2_aligned: list
    costs: "numpy.ndarray"
    scores: "numpy.ndarray"
    seeds: list
    scoring_mat: dict
    costing_mat: dict
    gap_open_score: int
    gap_open_cost: int

    def result(self, k, t):
        """Sample t of pair k as an AlignmentResults (output=None), with the batch's matrices."""
        return AlignmentResults(self.seq_1_aligned[k][t], self.middle_part[k][t], self.seq_2_aligned[k][t],
                                int(self.costs[k]), int(self.scores[k]), self.scoring_mat, self.costing_mat,
                                self.gap_open_score, self.gap_open_cost, None)

    def distinct(self, k):
        """Pair k's different alignments with how many samples gave each: a list of ((seq_1_aligned, middle_part,
        seq_2_aligned), count) in order of first appearance."""
        counts = {}
        for key in zip(self.seq_1_aligned[k], self.middle_part[k], self.seq_2_aligned[k]):
            counts[key] = counts.get(key, 0) + 1
        return list(counts.items())


class BatchCounts(NamedTuple):
    """The number of co-optimal alignments of every pair (GlobalAligner.count_alignments): how many different
    alignments the traceback can return for the pair over all tie-breaks.  counts: numpy float64, shape (P,) -- the
    counts grow exponentially with the lengths, so they are doubles: the exact integer where exact[k] (counts[k] <
    2**53: every partial sum is a positive integer no larger than the total), the recurrence's double sum above, +inf
    past the double range; exact: numpy bool, shape (P,); the pair's cost and score in numpy int64 arrays; and the
    settings, as BatchScores reports them."""
    counts: "numpy.ndarray"
    exact: "numpy.ndarray"
    costs: "numpy.ndarray"
    scores: "numpy.ndarray"
    scoring_mat: dict
    costing_mat: dict
    gap_open_score: int
    gap_open_cost: int

    def count(self, k):
        """Pair k's count: a Python int when it is exact, else the float."""
        return int(self.counts[k]) if self.exact[k] else float(self.counts[k])


class BatchRanked(NamedTuple):
    """Co-optimal alignments of every pair by rank (GlobalAligner.alignments_by_rank, enumerate_alignments,
    sample_alignments_uniform): per pair a list with one string per requested rank, for each of the three lines; the
    pair's cost and score in numpy int64 arrays of shape (P,); per pair the uint64 array of the ranks asked for; counts:
    numpy uint64, shape (P,), min(the pair's number of co-optimal alignments, 2**64 - 1) -- every rank below it is exact
    whatever the true count; saturated: numpy bool, counts == 2**64 - 1; and the settings, as BatchAlignments reports
    them."""
    seq_1_aligned: list
    middle_part: list
    seq_2_aligned: list
    costs: "numpy.ndarray"
    scores: "numpy.ndarray"
    ranks: list
    counts: "numpy.ndarray"
    saturated: "numpy.ndarray"
    scoring_mat: dict
    costing_mat: dict
    gap_open_score: int
    gap_open_cost: int

    def result(self, k, t):
        """Entry t of pair k (the alignment of rank ranks[k][t]) as an AlignmentResults (output=None), with the batch's
        matrices."""
        return AlignmentResults(self.seq_1_aligned[k][t], self.middle_part[k][t], self.seq_2_aligned[k][t],
                                int(self.costs[k]), int(self.scores[k]), self.scoring_mat, self.costing_mat,
                                self.gap_open_score, self.gap_open_cost, None)

    def complete(self, k):
        """Whether pair k's entries are the pair's whole family of co-optimal alignments, in rank order: its count is not
        saturated and ranks[k] is exactly 0 .. counts[k] - 1."""
        n = int(self.counts[k])
        r = self.ranks[k]
        return not bool(self.saturated[k]) and len(r) == n and all(int(x) == q for q, x in enumerate(r))


class BatchSupport(NamedTuple):
    """Match support of every pair (GlobalAligner.match_support): support, per pair a numpy float64 array of shape
    (m, n) whose entry [i, j] is the number of the pair's co-optimal alignments that align letter i of seq_1 with letter
    j of seq_2 (0-based) in one column; counts, exact, costs and scores as BatchCounts has them -- where exact[k] every
    support of pair k is an exact integer, above 2**53 it is the recurrence's double; seqs_1, seqs_2: the pairs'
    upper-cased sequences; and the settings, as BatchScores reports them.  The methods are plain numpy on these."""
    support: list
    counts: "numpy.ndarray"
    exact: "numpy.ndarray"
    costs: "numpy.ndarray"
    scores: "numpy.ndarray"
    seqs_1: list
    seqs_2: list
    scoring_mat: dict
    costing_mat: dict
    gap_open_score: int
    gap_open_cost: int

    def count(self, k):
        """Pair k's count: a Python int when it is exact, else the float."""
        return int(self.counts[k]) if self.exact[k] else float(self.counts[k])

    def fraction(self, k):
        """support[k] / counts[k]: per cell the share of the family that has the column."""
        return self.support[k] / self.counts[k]

    def core(self, k):
        """The columns every co-optimal alignment of pair k has: an int64 array (r, 2) of the 0-based (i, j) with
        support == counts[k], in increasing i (and with it j: they lie on one path)."""
        import numpy as np
        return np.argwhere(self.support[k] == self.counts[k]).astype(np.int64).reshape(-1, 2)

    def unaligned_1(self, k):
        """Per letter of seq_1: the number of members in which it faces a gap, counts[k] - support[k].sum(axis=1) (a
        member has the letter in one column: with one letter of seq_2 or with a gap); an exact integer where
        exact[k]."""
        return self.counts[k] - self.support[k].sum(axis=1)

    def unaligned_2(self, k):
        """Per letter of seq_2: the number of members in which it faces a gap, counts[k] - support[k].sum(axis=0)."""
        return self.counts[k] - self.support[k].sum(axis=0)

    def column_support(self, k, seq_1_aligned, seq_2_aligned):
        """Per column of an alignment of pair k (its two lines, gaps as '-'): the fraction of the family that has the
        column -- fraction(k) at a column of two letters, the unaligned fraction of the letter at a gap column (the
        share in which that letter faces a gap, wherever the gap lies).  -> float64 array, one entry per column.
        ValueError if the lines differ in length, have a column of two gaps, or are not, dashes removed, the pair's
        upper-cased sequences."""
        import numpy as np
        a, b = str(seq_1_aligned), str(seq_2_aligned)
        if len(a) != len(b):
            raise ValueError("the aligned lines differ in length")
        if a.replace("-", "") != self.seqs_1[k] or b.replace("-", "") != self.seqs_2[k]:
            raise ValueError(f"the lines are not an alignment of pair {k}'s sequences")
        frac = self.fraction(k)
        gap_1, gap_2 = self.unaligned_1(k) / self.counts[k], self.unaligned_2(k) / self.counts[k]
        out = np.zeros(len(a), dtype=np.float64)
        i = j = 0
        for c, (x, y) in enumerate(zip(a, b)):
            if x == "-" and y == "-":
                raise ValueError(f"column {c} holds two gaps")
            if x == "-":
                out[c] = gap_2[j]
                j += 1
            elif y == "-":
                out[c] = gap_1[i]
                i += 1
            else:
                out[c] = frac[i, j]
                i += 1
                j += 1
        return out
