#!/usr/bin/env python3
"""Optimal global alignment on MI355X -- drop-in for globalign's hot path.

Public surface (mirrors iamgiddyaboutgit/globalign src/globalign/globaligner.py):

  find_global_alignment(...) -> AlignmentResults        globaligner.py:132-314
  make_dp_array / dp_array_forward / dp_array_backward   globaligner.py:756-821, 366-392, 395-593
  main()  (the `globaligner` CLI)                        globaligner.py:23-129
plus GlobalAligner, a reusable façade bound to one GPU that can lift the
reference's m*n < 2e7 cap.

The three DP functions run on the GPU through the C ABI in
include/globalign_amd.h; there is no CPU fallback.  Tie-breaking consumes the
process-global ``random`` state exactly like the reference (18
``random.choice`` calls per traceback step), so with the same
``random.seed`` the alignment strings are identical.
"""
import argparse
import math
import numbers
import random
import sys
import types
from pathlib import Path

import numpy as np

from . import _native
from .results import (AlignmentResults, BatchAlignments, BatchCounts, BatchRanked, BatchSamples, BatchScores, BatchSupport,
                      final_cost_to_score)
from .scoring import MAX_SEQ_LEN_PROD, get_max_val, validate_and_transform_args

__version__ = "0.1.0"


def _mt_words():
    st = random.getstate()
    return np.array(st[1], dtype=np.uint32)


def _set_mt_words(words):
    # only the MT words move: random.choice leaves gauss_next (the state's third item) alone
    st = random.getstate()
    random.setstate((st[0], tuple(int(x) for x in words), st[2]))


class GlobalAligner:
    """Reusable aligner on one GPU or several.

    ``GlobalAligner(**settings).align(seq_1, seq_2)`` accepts the same keyword
    settings as find_global_alignment (scores, costs, matrix name/path, gap
    options) and returns an AlignmentResults.  ``max_seq_len_prod=None``
    lifts the reference's m*n < 2e7 API cap (the device path is sized for
    100k x 100k and beyond); ``traceback=False`` returns the score only.
    ``devices=[0, 1, ...]`` cuts seq_2's columns into one slab per listed GPU
    of this process (distributed.align_devices: each slab's fill writes its right
    edge straight into its neighbour's GPU memory over xGMI while both fills
    run, the walk is handed right to left);
    the result is identical to the one-GPU result.  For one process per GPU
    use globalign_amd.distributed (torch.distributed / RCCL).
    """

    def __init__(self, scoring_mat_name=None, scoring_mat_path=None, match_score=None, mismatch_score=None,
                 mismatch_cost=None, gap_open_score=None, gap_open_cost=None, gap_extension_score=None,
                 gap_extension_cost=None, device=0, max_seq_len_prod=MAX_SEQ_LEN_PROD, traceback=True, devices=None):
        self.settings = dict(scoring_mat_name=scoring_mat_name, scoring_mat_path=scoring_mat_path,
                             match_score=match_score, mismatch_score=mismatch_score, mismatch_cost=mismatch_cost,
                             gap_open_score=gap_open_score, gap_open_cost=gap_open_cost,
                             gap_extension_score=gap_extension_score, gap_extension_cost=gap_extension_cost)
        self.devices = [int(d) for d in devices] if devices is not None else [int(device)]
        if not self.devices:
            raise ValueError("devices must name at least one GPU")
        self.device = self.devices[0]
        self.max_seq_len_prod = max_seq_len_prod
        self.traceback = traceback

    def align(self, seq_1=None, seq_2=None, input_fasta=None, output=None):
        good = validate_and_transform_args(input_fasta, output, seq_1, seq_2, max_seq_len_prod=self.max_seq_len_prod,
                                           **self.settings)
        return _align_validated(good, device=self.device, traceback=self.traceback, devices=self.devices)


    def align_repeated(self, seq_1, seq_2, count):
        """`count` alignments of one pair, as `count` consecutive find_global_alignment calls make them: each
        starts from the global random state the previous one left, so the tie-breaks -- and with them the
        co-optimal alignment returned -- differ from call to call exactly as in the reference.  On one GPU
        the walk of alignment k runs beside the fill of alignment k+1 (ga_problem_align_many).
        -> list of AlignmentResults."""
        good = validate_and_transform_args(None, None, seq_1, seq_2, max_seq_len_prod=self.max_seq_len_prod,
                                           **self.settings)
        s1, s2, scoring_mat, costing_mat, gos, goc, output = good
        if int(count) <= 0:
            return []  # a loop of zero find_global_alignment calls
        if len(self.devices) > 1 or not self.traceback or min(len(s1), len(s2)) < 2:
            # (degenerate lengths may raise the reference's IndexError mid-way: one call at a time)
            return [_align_validated(good, device=self.device, traceback=self.traceback, devices=self.devices)
                    for _ in range(int(count))]
        tables = _native.CostTables(costing_mat, goc)
        eng = _native.default_engine(self.device)
        eng.load(tables.codes(s1), tables.codes(s2), tables)
        mt0 = _mt_words()
        runs, mt = eng.align_many(mt0, s1, s2, int(count))
        if any(status == _native.GA_TB_INDEX_ERROR for _, _, status in runs):
            # consecutive reference calls stop at the first IndexError, with the random state that call
            # left: replay them one at a time from the starting state (never reached for min(m, n) >= 2)
            _set_mt_words(mt0)
            return [_align_validated(good, device=self.device, traceback=True) for _ in range(int(count))]
        _set_mt_words(mt)
        out = []
        for cost, (a, mid, b), status in runs:
            score = final_cost_to_score(cost=cost, m=len(s1), n=len(s2), max_score=get_max_val(scoring_mat))
            out.append(AlignmentResults(a, mid, b, cost, score, scoring_mat, costing_mat, gos, goc, output))
        return out

    def score_pairs(self, seqs_1, seqs_2):
        """Costs and scores of seqs_1[k] aligned with seqs_2[k] for every k, in one call: no alignment strings, no
        use of the global random state.  costs[k] / scores[k] equal .cost / .score of
        GlobalAligner(traceback=False, ...).align(seqs_1[k], seqs_2[k]) under this aligner's settings.
        -> BatchScores with arrays of shape (len(seqs_1),)."""
        seqs_1, seqs_2 = list(seqs_1), list(seqs_2)
        if len(seqs_1) != len(seqs_2):
            raise ValueError(f"score_pairs needs as many first as second sequences, got {len(seqs_1)} and "
                             f"{len(seqs_2)}")
        P = len(seqs_1)
        return self._score_batch(seqs_1 + seqs_2, np.arange(P, dtype=np.int64), np.arange(P, 2 * P, dtype=np.int64),
                                 (P,))

    def score_matrix(self, seqs, seqs_2=None):
        """Costs and scores of every seqs[i] aligned with every seqs_2[j] (seqs_2=None: seqs against itself).  All
        N1 x N2 entries are computed: costs are not symmetric in general (the vertical and horizontal gap costs of
        a transformed scoring matrix differ when its maximum is odd).  -> BatchScores with (N1, N2) arrays."""
        seqs = list(seqs)
        rows = np.arange(len(seqs), dtype=np.int64)
        if seqs_2 is None:
            cols = rows
        else:
            seqs_2 = list(seqs_2)
            cols = np.arange(len(seqs), len(seqs) + len(seqs_2), dtype=np.int64)
            seqs = seqs + seqs_2
        return self._score_batch(seqs, np.repeat(rows, len(cols)), np.tile(cols, len(rows)), (len(rows), len(cols)))

    def align_pairs(self, seqs_1, seqs_2, seeds=0, tables="host"):
        """Alignments of seqs_1[k] with seqs_2[k] for every k, strings included, in one call.  Pair k is aligned under
        a random seed of its own: ``seeds`` is an int base (pair k uses base + k) or a sequence of one int per pair,
        each in [0, 2**64).  Pair k's strings, cost and score are those of ``random.seed(s_k)`` followed by
        ``GlobalAligner(**settings).align(seqs_1[k], seqs_2[k])``, whatever the batch's order or composition; the
        process-global ``random`` state is left as it was.  Validation is score_pairs's.  A pair for which the single
        call raises the reference's IndexError (possible only with a one-letter sequence) makes the call raise
        IndexError("pair <k>: string index out of range") for the lowest such k.
        ``tables`` says where the pairs' tie-break tables are made: "host" (a few CPU threads) or "device" (generated
        on the GPU ahead of the walks, so the call's time does not depend on the host's cores); the results are the
        same byte for byte.
        -> BatchAlignments."""
        seeds, b, route = self._strings_batch("align_pairs", seqs_1, seqs_2, tables, lambda P: _pair_seeds(seeds, P))
        if b is None:
            e = self._empty_batch((0,))
            return BatchAlignments([], [], [], e.costs, e.scores, *e[2:])
        eng = _native.default_engine(self.device)
        costs, status, lengths, offsets, bufs = eng.batch_align(b.codes, b.seq_off, b.pair_a, b.pair_b, b.tables, seeds,
                                                                np.frombuffer(b.text, dtype=np.uint8), b.pair_max_cost,
                                                                **route)
        failed = np.flatnonzero(status == _native.GA_TB_INDEX_ERROR)
        if failed.size:
            raise IndexError(f"pair {int(failed[0])}: string index out of range")  # the reference's, SURVEY A.5
        strings = _cut_strings(bufs, offsets, lengths)
        return BatchAlignments(strings[0], strings[1], strings[2], costs, b.scores(costs), b.scoring_mat, b.costing_mat,
                               b.gap_open_score, b.gap_open_cost)

    def sample_alignments(self, seqs_1, seqs_2, samples=None, seeds=0, tables="host"):
        """Many alignments of seqs_1[k] with seqs_2[k] for every k, each under a random seed of its own, from ONE fill
        of the pair: the reference breaks traceback ties with random.choice, so a pair has a family of co-optimal
        alignments, and only the walk depends on the seed.  ``samples`` is an int S >= 1 (every pair gets S) or one
        int >= 1 per pair.  ``seeds`` is an int base -- the samples are numbered flat in pair order, f = 0, 1, ...,
        and sample f uses base + f -- or a sequence with, per pair, the sequence of that pair's seeds (``samples`` may
        then be None; if given it must agree).  Every effective seed lies in [0, 2**64).
        Sample t of pair k is, byte for byte, what ``random.seed(s_kt)`` followed by
        ``GlobalAligner(**settings).align(seqs_1[k], seqs_2[k])`` returns -- entry f of align_pairs on the lists with
        every pair repeated once per sample; the process-global ``random`` state is left as it was.  Validation, the
        IndexError of a one-letter pair (raised for the lowest pair any of whose samples raises it) and ``tables`` are
        align_pairs's.
        -> BatchSamples."""
        (counts, flat), b, route = self._strings_batch("sample_alignments", seqs_1, seqs_2, tables,
                                                       lambda P: _sample_seeds(samples, seeds, P))
        if b is None:
            e = self._empty_batch((0,))
            return BatchSamples([], [], [], e.costs, e.scores, [], *e[2:])
        sample_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        eng = _native.default_engine(self.device)
        costs, status, lengths, offsets, bufs = eng.batch_sample(b.codes, b.seq_off, b.pair_a, b.pair_b, b.tables,
                                                                 sample_off, flat, np.frombuffer(b.text, dtype=np.uint8),
                                                                 b.pair_max_cost, **route)
        failed = np.flatnonzero(status == _native.GA_TB_INDEX_ERROR)
        if failed.size:
            k = int(np.searchsorted(sample_off, failed[0], side="right")) - 1
            raise IndexError(f"pair {k}: string index out of range")  # the reference's, SURVEY A.5
        cut = list(zip(sample_off[:-1].tolist(), sample_off[1:].tolist()))
        strings = [[flat_strings[x:y] for x, y in cut] for flat_strings in _cut_strings(bufs, offsets, lengths)]
        return BatchSamples(strings[0], strings[1], strings[2], costs, b.scores(costs),
                            [flat[x:y].copy() for x, y in cut], b.scoring_mat, b.costing_mat,
                            b.gap_open_score, b.gap_open_cost)

    def count_alignments(self, seqs_1, seqs_2):
        """The number of co-optimal alignments of seqs_1[k] with seqs_2[k] for every k: how many different
        (seq_1_aligned, middle_part, seq_2_aligned) results ``align`` can return for the pair over all outcomes of the
        reference's random tie-breaks -- what ``sample_alignments`` draws from, so ``len(distinct(k))`` of any sample
        run is at most ``counts[k]``.  The counts come from one fill of the pair and a path count over its traceback
        words on the GPU; the process-global ``random`` state is not touched.  Validation is align_pairs's.  A pair
        with a one-letter sequence has no count (the reference's traceback is not a path walk there) and raises
        ValueError for the lowest such pair, as does a pair whose traceback words do not fit the device's budget.
        -> BatchCounts."""
        _, b, _ = self._strings_batch("count_alignments", seqs_1, seqs_2, "host", lambda P: None)
        if b is None:
            e = self._empty_batch((0,))
            return BatchCounts(np.zeros(0, dtype=np.float64), np.zeros(0, dtype=bool), e.costs, e.scores, *e[2:])
        lens = np.diff(b.seq_off)
        short = np.flatnonzero(np.minimum(lens[b.pair_a], lens[b.pair_b]) < 2)
        if short.size:
            raise ValueError(f"pair {int(short[0])}: count_alignments needs sequences of at least two letters")
        eng = _native.default_engine(self.device)
        costs, counts = eng.batch_count(b.codes, b.seq_off, b.pair_a, b.pair_b, b.tables, b.pair_max_cost)
        return BatchCounts(counts, counts < 2.0 ** 53, costs, b.scores(costs), b.scoring_mat, b.costing_mat,
                           b.gap_open_score, b.gap_open_cost)

    def match_support(self, seqs_1, seqs_2):
        """For every pair and every letter i of seqs_1[k] and letter j of seqs_2[k]: how many of the pair's co-optimal
        alignments (``count_alignments`` says how many there are) align the two in one column.  ``support[k][i, j] ==
        counts[k]`` marks a column every co-optimal alignment has, 0 one that none has; ``fraction``, ``core``,
        ``unaligned_1`` / ``unaligned_2`` and ``column_support`` of the result read the matrix.  The supports are exact
        integers in float64 where ``exact[k]`` (counts[k] < 2**53) and the same recurrence's doubles above.  They come
        from one fill of the pair and two passes over its traceback words on the GPU -- the number of paths below every
        state, then the number of walk prefixes above it -- with no enumeration and no sampling; the process-global
        ``random`` state is not touched.  Validation and refusals are count_alignments's; a pair whose count is not
        finite (+inf, past the double range) raises ValueError, the lowest such pair named.
        -> BatchSupport."""
        _, b, _ = self._strings_batch("match_support", seqs_1, seqs_2, "host", lambda P: None)
        if b is None:
            e = self._empty_batch((0,))
            return BatchSupport([], np.zeros(0, dtype=np.float64), np.zeros(0, dtype=bool), e.costs, e.scores, [], [],
                                *e[2:])
        lens = np.diff(b.seq_off)
        short = np.flatnonzero(np.minimum(lens[b.pair_a], lens[b.pair_b]) < 2)
        if short.size:
            raise ValueError(f"pair {int(short[0])}: match_support needs sequences of at least two letters")
        eng = _native.default_engine(self.device)
        costs, counts, offsets, flat = eng.batch_support(b.codes, b.seq_off, b.pair_a, b.pair_b, b.tables, b.pair_max_cost)
        support = [flat[offsets[k]:offsets[k + 1]].reshape(int(lens[b.pair_a[k]]), int(lens[b.pair_b[k]]))
                   for k in range(len(b.pair_a))]
        text = b.text.decode("latin-1")
        seqs = [text[b.seq_off[s]:b.seq_off[s + 1]] for s in range(len(b.seq_off) - 1)]
        return BatchSupport(support, counts, counts < 2.0 ** 53, costs, b.scores(costs), [seqs[a] for a in b.pair_a],
                            [seqs[q] for q in b.pair_b], b.scoring_mat, b.costing_mat, b.gap_open_score, b.gap_open_cost)

    def alignments_by_rank(self, seqs_1, seqs_2, ranks):
        """The co-optimal alignments of seqs_1[k] with seqs_2[k] that ``ranks[k]`` names, for every k.  The reference
        breaks traceback ties with random.choice, so a pair has a family of co-optimal alignments (``count_alignments``
        says how many).  They are ordered by the levels the traceback emits, from the alignment's last column
        backwards: at the first column where two of them differ, a column of both letters comes before a gap in seq_1,
        and that before a gap in seq_2; the forced tail after the first row or column adds nothing.  Rank r is the
        r-th alignment of that order, from 0.  ``ranks`` holds one sequence of ints per pair (it may be empty: the pair
        is only counted), each in [0, 2**64 - 1).  The GPU fills the pair once, keeps the number of paths below every
        state of the traceback, and walks down from the last cell entering, at every tie, the branch whose path count
        contains the rank; no random number is drawn and the process-global ``random`` state is not touched.
        ``counts[k]`` is min(the pair's count, 2**64 - 1): the counts saturate there, and every rank below counts[k] is
        exact all the same.  Validation is count_alignments's; a rank that is not below its pair's count raises
        ValueError for the lowest pair and slot.
        -> BatchRanked."""
        return self._ranked("alignments_by_rank", seqs_1, seqs_2, ranks)

    def _ranked(self, method, seqs_1, seqs_2, ranks):
        """alignments_by_rank under the name `method` (the name in the messages)."""
        _, b, _ = self._strings_batch(method, seqs_1, seqs_2, "host", lambda P: None)
        per_pair = _rank_lists(ranks, 0 if b is None else len(b.pair_a))
        if b is None:
            e = self._empty_batch((0,))
            return BatchRanked([], [], [], e.costs, e.scores, [], np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=bool),
                               *e[2:])
        lens = np.diff(b.seq_off)
        short = np.flatnonzero(np.minimum(lens[b.pair_a], lens[b.pair_b]) < 2)
        if short.size:
            raise ValueError(f"pair {int(short[0])}: {method} needs sequences of at least two letters")
        rank_off = np.concatenate([[0], np.cumsum([len(r) for r in per_pair])]).astype(np.int64)
        flat = np.concatenate(per_pair) if per_pair else np.zeros(0, dtype=np.uint64)
        eng = _native.default_engine(self.device)
        costs, counts, status, lengths, offsets, bufs = eng.batch_rank(b.codes, b.seq_off, b.pair_a, b.pair_b, b.tables,
                                                                       rank_off, flat,
                                                                       np.frombuffer(b.text, dtype=np.uint8),
                                                                       b.pair_max_cost)
        failed = np.flatnonzero(status != 0)
        if failed.size:
            k = int(np.searchsorted(rank_off, failed[0], side="right")) - 1
            raise ValueError(f"pair {k}: rank {int(flat[failed[0]])} is not below the pair's count {int(counts[k])}")
        cut = list(zip(rank_off[:-1].tolist(), rank_off[1:].tolist()))
        strings = [[flat_strings[x:y] for x, y in cut] for flat_strings in _cut_strings(bufs, offsets, lengths)]
        return BatchRanked(strings[0], strings[1], strings[2], costs, b.scores(costs), per_pair, counts,
                           counts == np.uint64(2 ** 64 - 1), b.scoring_mat, b.costing_mat, b.gap_open_score,
                           b.gap_open_cost)

    def enumerate_alignments(self, seqs_1, seqs_2, limit=1024):
        """The first min(count, limit) co-optimal alignments of every pair in rank order (alignments_by_rank has the
        order): the pair's whole family where ``complete(k)`` says so.  ``limit`` is an int >= 1.  Two
        alignments_by_rank calls: one without ranks for the counts, one for the ranks 0 .. min(counts[k], limit) - 1, so
        the pairs are filled and their count tables made twice -- that keeps the engine to one mode.
        -> BatchRanked."""
        if not isinstance(limit, numbers.Integral) or isinstance(limit, bool):
            raise TypeError("limit must be an int")
        if int(limit) < 1:
            raise ValueError("limit must be at least 1")
        seqs_1, seqs_2 = list(seqs_1), list(seqs_2)
        counted = self._ranked("enumerate_alignments", seqs_1, seqs_2, [()] * min(len(seqs_1), len(seqs_2)))
        return self._ranked("enumerate_alignments", seqs_1, seqs_2,
                            [range(min(int(c), int(limit))) for c in counted.counts])

    def sample_alignments_uniform(self, seqs_1, seqs_2, samples, seed=0):
        """Co-optimal alignments of every pair drawn uniformly from the pair's family: every one of its counts[k]
        alignments is as likely as any other, unlike ``sample_alignments``, whose random.choice per traceback step draws
        an alignment through many ties far less often than one through few.  ``samples`` is an int S >= 1 (every pair
        gets S) or one int >= 1 per pair; ``seed`` an int.  The ranks are drawn by ``rng = random.Random(seed)``, pair by
        pair and sample by sample, as ``rng.randrange(counts[k])``, and handed to one alignments_by_rank call (a call
        without ranks ahead of it gets the counts): the result is reproducible, and the process-global ``random`` state
        is not touched.  A pair whose count is saturated (2**64 - 1 or more alignments) raises ValueError, the lowest
        such pair first: a u64 rank cannot index its family.
        -> BatchRanked."""
        seqs_1, seqs_2 = list(seqs_1), list(seqs_2)
        if not isinstance(seed, numbers.Integral):
            raise TypeError("seed must be an int")
        P = min(len(seqs_1), len(seqs_2))
        # (unequal lists are the first call's to refuse)
        per_pair = _sample_seeds(samples, 0, P)[0] if len(seqs_1) == len(seqs_2) else None
        counted = self._ranked("sample_alignments_uniform", seqs_1, seqs_2, [()] * P)
        full = np.flatnonzero(counted.saturated)
        if full.size:
            raise ValueError(f"pair {int(full[0])}: the count is saturated (2**64 - 1 or more co-optimal alignments), "
                             "a uniform rank cannot be drawn")
        rng = random.Random(int(seed))
        ranks = [[rng.randrange(int(counted.counts[k])) for _ in range(per_pair[k])] for k in range(P)]
        return self._ranked("sample_alignments_uniform", seqs_1, seqs_2, ranks)

    def _strings_batch(self, method, seqs_1, seqs_2, tables, seeds_of):
        """The front half of align_pairs and sample_alignments (`method`: the name in the messages): the checks in their
        order, the seeds by seeds_of(P), and the batch.  -> (seeds, the _prepare_batch namespace or None for no pairs,
        the engine call's route arguments)."""
        if tables not in ("host", "device"):
            raise ValueError(f"tables must be 'host' or 'device', not {tables!r}")
        seqs_1, seqs_2 = list(seqs_1), list(seqs_2)
        if len(seqs_1) != len(seqs_2):
            raise ValueError(f"{method} needs as many first as second sequences, got {len(seqs_1)} and "
                             f"{len(seqs_2)}")
        if not self.traceback:
            raise ValueError(f"{method} returns alignment strings; an aligner made with traceback=False scores "
                             "batches with score_pairs")
        if len(self.devices) > 1:
            raise ValueError(f"{method} runs on one GPU; this aligner was made with devices={self.devices}")
        P = len(seqs_1)
        seeds = seeds_of(P)
        # (the host route is the engine's call as it always was; only the device route names itself)
        route = {} if tables == "host" else {"rng_tables": tables}
        if P == 0:
            return seeds, None, route
        b = self._prepare_batch(seqs_1 + seqs_2, np.arange(P, dtype=np.int64), np.arange(P, 2 * P, dtype=np.int64))
        if b.text is None:
            raise ValueError(f"{method} takes sequences of one-byte (latin-1) letters")
        return seeds, b, route

    def _empty_batch(self, shape):
        """No pairs: empty arrays, no launch.  The option checks still run, through the single call's validation of
        a placeholder pair; the matrices are reported only where they do not depend on the sequences (a named or
        file matrix)."""
        empty = np.zeros(shape, dtype=np.int64)
        from_matrix = self.settings["scoring_mat_name"] is not None or self.settings["scoring_mat_path"] is not None
        try:
            _, _, smat, cmat, gos, goc, _ = validate_and_transform_args(None, None, "A", "A", max_seq_len_prod=None,
                                                                        **self.settings)
        except RuntimeError as e:
            if not (from_matrix and str(e).startswith("common_alphabet contains values")):
                raise
            # (a file matrix without the placeholder's letter: every option check had passed by then)
            return BatchScores(empty, empty.copy(), None, None, None, None)
        if not from_matrix:
            smat = cmat = None
        return BatchScores(empty, empty.copy(), smat, cmat, gos, goc)

    def _score_batch(self, seqs, pair_a, pair_b, shape):
        """seqs[pair_a[k]] against seqs[pair_b[k]] for every k.  Validation is the single call's, per pair and in
        pair order, before any engine exists; the options and the score -> cost transform run once."""
        if len(self.devices) > 1:
            raise ValueError("score_pairs / score_matrix run on one GPU; this aligner was made with devices="
                             f"{self.devices}")
        if len(pair_a) == 0:
            return self._empty_batch(shape)
        b = self._prepare_batch(seqs, pair_a, pair_b)
        eng = _native.default_engine(self.device)
        costs = eng.batch_costs(b.codes, b.seq_off, pair_a, pair_b, b.tables, b.pair_max_cost)
        return BatchScores(costs.reshape(shape), b.scores(costs).reshape(shape), b.scoring_mat, b.costing_mat,
                           b.gap_open_score, b.gap_open_cost)

    def _prepare_batch(self, seqs, pair_a, pair_b):
        """What a batch call needs before it asks for an engine (score_pairs, score_matrix, align_pairs): every pair
        validated as the single call validates it, the batch's tables and codes, and the per-pair quantities of
        one-letter pairs.  -> a namespace: pair_a, pair_b, codes, seq_off, tables, pair_max_cost, text (the
        upper-cased sequences joined, as latin-1 bytes, or None), the matrices and gap-open values, and
        scores(costs)."""
        try:
            joined = "".join(seqs)
        except TypeError:
            raise TypeError("sequences must be str") from None

        def single_call(k):
            return validate_and_transform_args(None, None, seqs[pair_a[k]], seqs[pair_b[k]],
                                               max_seq_len_prod=self.max_seq_len_prod, **self.settings)

        # pair 0 as the single call validates it: its own faults first, then whatever does not depend on the sequences
        # (option combinations, the matrix file)
        _, _, scoring_mat, costing_mat, gap_open_score, gap_open_cost, _ = single_call(0)
        from_matrix = self.settings["scoring_mat_name"] is not None or self.settings["scoring_mat_path"] is not None
        # The other pairs: find the first one the single call would refuse, and let the single call refuse it.  The
        # whole batch is looked at as one string (one upper(), one byte histogram), the sequences one by one only
        # when something in it is wrong.
        raw_len = np.fromiter(map(len, seqs), dtype=np.int64, count=len(seqs))
        upper = joined.upper()
        lens = raw_len
        if len(upper) != len(joined):  # (a letter whose upper case is longer: per sequence)
            lens = np.fromiter((len(s.upper()) for s in seqs), dtype=np.int64, count=len(seqs))
        # what the batch holds beyond pair 0's tables (its alphabet, or the matrix's letters): other letters, and '-'
        keys = set(scoring_mat.keys()) - {"-"}
        try:
            text = upper.encode("latin-1")
            extra = set(text.translate(None, bytes(ord(k) for k in keys if len(k) == 1 and ord(k) < 256)).decode("latin-1"))
        except UnicodeEncodeError:
            text = None
            extra = set(upper) - keys
        dash = "-" in extra
        extra.discard("-")
        unknown = extra if from_matrix else set()
        prod = raw_len[pair_a] * raw_len[pair_b]
        bad = prod == 0
        if self.max_seq_len_prod is not None:
            bad |= ~(prod < self.max_seq_len_prod)
        if dash or unknown:
            flagged = np.fromiter(("-" in s or not unknown.isdisjoint(s.upper()) for s in seqs), dtype=bool,
                                  count=len(seqs))
            bad |= flagged[pair_a] | flagged[pair_b]
        if bad.any():
            k = int(np.argmax(bad))
            single_call(k)
            raise RuntimeError(f"pair {k} failed validation")  # (the single call raises before this)
        if not from_matrix and extra:
            # match / mismatch tables over the whole batch's alphabet: they are constant off the diagonal, so every
            # entry a pair reads is what its own alphabet's tables hold (the maximum is another matter, below)
            alphabet = "".join(sorted(keys | extra))
            _, _, scoring_mat, costing_mat, gap_open_score, gap_open_cost, _ = validate_and_transform_args(
                None, None, alphabet, alphabet, max_seq_len_prod=None, **self.settings)
        tables = _native.CostTables(costing_mat, gap_open_cost)
        seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        # A pair made of ONE letter: the single call builds its match / mismatch matrices over that letter alone, and
        # they hold no mismatch entry, so their maxima -- the sentinel big = (max_cost + 1) * max(m, n) and the
        # score's deltas come from them -- differ from the batch tables'.  Such pairs get their own.
        max_score = get_max_val(scoring_mat)
        delta_d, delta_i, pair_max_cost = math.floor(max_score / 2), math.ceil(max_score / 2), None
        if not from_matrix and len(keys | extra) > 1:
            letter = _one_letter_sequences(upper, text, seq_off)
            one = (letter[pair_a] >= 0) & (letter[pair_a] == letter[pair_b])
            if one.any():
                x = upper[0]
                _, _, smat_1, cmat_1, _, _, _ = validate_and_transform_args(None, None, x, x, max_seq_len_prod=None,
                                                                            **self.settings)
                pair_max_cost = np.where(one, int(get_max_val(cmat_1)), tables.max_cost).astype(np.int32)
                b1 = get_max_val(smat_1)
                delta_d = np.where(one, math.floor(b1 / 2), delta_d).astype(np.int64)
                delta_i = np.where(one, math.ceil(b1 / 2), delta_i).astype(np.int64)
        if text is not None:
            lut = bytearray(256)
            for ch, code in tables.code.items():
                if len(ch) == 1 and ord(ch) < 256:
                    lut[ord(ch)] = code
            codes = np.frombuffer(text.translate(bytes(lut)), dtype=np.uint8)
        else:
            codes = np.fromiter((tables.code[ch] for ch in upper), dtype=np.uint8, count=len(upper))

        def scores(costs):
            return np.asarray(final_cost_to_score(cost=costs, m=lens[pair_a], n=lens[pair_b], max_score=max_score,
                                                  delta_d=delta_d, delta_i=delta_i), dtype=np.int64)

        return types.SimpleNamespace(pair_a=pair_a, pair_b=pair_b, codes=codes, seq_off=seq_off, tables=tables,
                                     pair_max_cost=pair_max_cost, text=text, scoring_mat=scoring_mat,
                                     costing_mat=costing_mat, gap_open_score=gap_open_score,
                                     gap_open_cost=gap_open_cost, scores=scores)


def _cut_strings(bufs, offsets, lengths):
    """The engine's three output buffers as three lists of strings: slot f's are the lengths[f] bytes at offsets[f]."""
    lo, hi = offsets[:-1].tolist(), (offsets[:-1] + lengths).tolist()
    return [[t[x:y] for x, y in zip(lo, hi)] for t in (buf.tobytes().decode("latin-1") for buf in bufs)]


def _pair_seeds(seeds, P):
    """align_pairs's seeds as a uint64 array of P entries: an int base (pair k: base + k) or one int per pair, every
    effective seed in [0, 2**64)."""
    if isinstance(seeds, numbers.Integral):
        values = [int(seeds), int(seeds) + max(P - 1, 0)]
    else:
        if isinstance(seeds, (str, bytes)):
            raise TypeError("seeds must be an int or a sequence of ints")
        try:
            values = list(seeds)
        except TypeError:
            raise TypeError("seeds must be an int or a sequence of ints") from None
        if len(values) != P:
            raise ValueError(f"align_pairs needs one seed per pair, got {len(values)} seeds for {P} pairs")
        if not all(isinstance(v, numbers.Integral) for v in values):
            raise TypeError("seeds must be ints")
        values = [int(v) for v in values]
    if any(v < 0 or v >= 2 ** 64 for v in values):
        raise ValueError("every seed must be in [0, 2**64)")
    if isinstance(seeds, numbers.Integral):
        return np.uint64(values[0]) + np.arange(P, dtype=np.uint64)
    return np.array(values, dtype=np.uint64)


def _rank_lists(ranks, P):
    """alignments_by_rank's ranks as a list of P uint64 arrays: one sequence of ints per pair (it may be empty), every
    rank in [0, 2**64 - 1)."""
    if isinstance(ranks, (str, bytes, numbers.Integral)):
        raise TypeError("ranks must be a sequence with one sequence of ints per pair")
    try:
        per_pair = list(ranks)
    except TypeError:
        raise TypeError("ranks must be a sequence with one sequence of ints per pair") from None
    if len(per_pair) != P:
        raise ValueError(f"ranks must have one entry per pair, got {len(per_pair)} for {P} pairs")
    out = []
    for k, own in enumerate(per_pair):
        if isinstance(own, (numbers.Integral, str, bytes)):
            raise TypeError("ranks must be a sequence with one sequence of ints per pair")
        try:
            own = list(own)
        except TypeError:
            raise TypeError("ranks must be a sequence with one sequence of ints per pair") from None
        if not all(isinstance(v, numbers.Integral) for v in own):
            raise TypeError(f"pair {k}: ranks must be ints")
        own = [int(v) for v in own]
        if any(v < 0 or v >= 2 ** 64 - 1 for v in own):
            raise ValueError(f"pair {k}: every rank must be in [0, 2**64 - 1)")
        out.append(np.array(own, dtype=np.uint64))
    return out


def _sample_seeds(samples, seeds, P):
    """sample_alignments's samples and seeds as (counts: P ints >= 1, flat: the uint64 seeds of all samples in pair
    order).  seeds is an int base (sample f of the flat numbering: base + f; samples is then needed) or one sequence
    of ints per pair; the type and range errors are _pair_seeds's."""
    counts = None
    if samples is not None:
        if isinstance(samples, numbers.Integral):
            counts = [int(samples)] * P
            if int(samples) < 1:
                raise ValueError("samples must be at least 1")
        else:
            if isinstance(samples, (str, bytes)):
                raise TypeError("samples must be an int or a sequence of ints")
            try:
                counts = list(samples)
            except TypeError:
                raise TypeError("samples must be an int or a sequence of ints") from None
            if len(counts) != P:
                raise ValueError(f"sample_alignments needs one sample count per pair, got {len(counts)} for {P} pairs")
            if not all(isinstance(v, numbers.Integral) for v in counts):
                raise TypeError("samples must be ints")
            counts = [int(v) for v in counts]
            if any(v < 1 for v in counts):
                raise ValueError("every pair needs at least 1 sample")
    if isinstance(seeds, numbers.Integral):
        if counts is None:
            if P:
                raise ValueError("samples is needed with an int seed base")
            counts = []
        return counts, _pair_seeds(seeds, sum(counts))
    if isinstance(seeds, (str, bytes)):
        raise TypeError("seeds must be an int or a sequence of sequences of ints")
    try:
        per_pair = list(seeds)
    except TypeError:
        raise TypeError("seeds must be an int or a sequence of sequences of ints") from None
    if len(per_pair) != P:
        raise ValueError(f"sample_alignments needs one sequence of seeds per pair, got {len(per_pair)} for {P} pairs")
    flat = []
    for k, own in enumerate(per_pair):
        if isinstance(own, (numbers.Integral, str, bytes)):
            raise TypeError("seeds must be an int or a sequence of sequences of ints")
        try:
            own = list(own)
        except TypeError:
            raise TypeError("seeds must be an int or a sequence of sequences of ints") from None
        if not own:
            raise ValueError(f"pair {k} needs at least 1 seed")
        flat.append(_pair_seeds(own, len(own)))
    if counts is not None and counts != [len(x) for x in flat]:
        raise ValueError("samples does not agree with the number of seeds given per pair")
    return [len(x) for x in flat], (np.concatenate(flat) if flat else np.zeros(0, dtype=np.uint64))


def _one_letter_sequences(upper, text, seq_off):
    """Per sequence of the batch (upper: all of them joined, text: the same as latin-1 bytes or None, seq_off: where
    each starts), the code point of its letter if it consists of one letter only, else -1."""
    starts, ends = seq_off[:-1], seq_off[1:]
    out = np.full(len(starts), -1, dtype=np.int64)
    if text is None:
        for s in range(len(starts)):
            u = upper[starts[s]:ends[s]]
            if u.count(u[0]) == len(u):
                out[s] = ord(u[0])
        return out
    arr = np.frombuffer(text, dtype=np.uint8)
    # only a sequence whose second letter equals its first can be one: the others are settled without a look
    maybe = arr[np.minimum(starts + 1, ends - 1)] == arr[starts]
    for s in np.flatnonzero(maybe):
        seg = text[starts[s]:ends[s]]
        if seg.count(seg[:1]) == len(seg):
            out[s] = seg[0]
    return out


def _align_validated(good, device=0, traceback=True, devices=None):
    seq_1, seq_2, scoring_mat, costing_mat, gap_open_score, gap_open_cost, output = good
    tables = _native.CostTables(costing_mat, gap_open_cost)
    if devices is not None and len(devices) > 1 and min(len(seq_1), len(seq_2)) >= 2 and len(seq_2) >= len(devices):
        from . import distributed
        cost, strings, status, mt = distributed.align_devices(devices, seq_1, seq_2, tables.codes(seq_1),
                                                              tables.codes(seq_2), tables, _mt_words(),
                                                              traceback=traceback)
        if traceback:
            _set_mt_words(mt)
            if status == _native.GA_TB_INDEX_ERROR:
                raise IndexError("string index out of range")
            a, mid, b = strings
        else:
            a = mid = b = None
        score = final_cost_to_score(cost=cost, m=len(seq_1), n=len(seq_2), max_score=get_max_val(scoring_mat))
        return AlignmentResults(a, mid, b, cost, score, scoring_mat, costing_mat, gap_open_score, gap_open_cost,
                                output)
    eng = _native.default_engine(device)
    eng.load(tables.codes(seq_1), tables.codes(seq_2), tables)
    if traceback:
        cost, (a, mid, b), status, mt = eng.align(_mt_words(), seq_1, seq_2)
        _set_mt_words(mt)  # the reference's random.choice calls advance the global state
        if status == _native.GA_TB_INDEX_ERROR:
            raise IndexError("string index out of range")  # reference behaviour for m==1 / n==1 walks (A.5)
    else:
        cost, _ = eng.fill(traceback=False)
        a = mid = b = None
    score = final_cost_to_score(cost=cost, m=len(seq_1), n=len(seq_2), max_score=get_max_val(scoring_mat))
    return AlignmentResults(a, mid, b, cost, score, scoring_mat, costing_mat, gap_open_score, gap_open_cost, output)


def find_global_alignment(input_fasta=None, output=None, seq_1=None, seq_2=None, scoring_mat_name=None,
                          scoring_mat_path=None, match_score=None, mismatch_score=None, mismatch_cost=None,
                          gap_open_score=None, gap_open_cost=None, gap_extension_score=None,
                          gap_extension_cost=None) -> AlignmentResults:
    """Optimal global alignment of seq_1 and seq_2 (Needleman-Wunsch / Gotoh affine gaps).

    Same arguments, defaults, validation and result as globalign's
    find_global_alignment; the DP fill and traceback run on the GPU."""
    good = validate_and_transform_args(input_fasta, output, seq_1, seq_2, scoring_mat_name, scoring_mat_path,
                                       match_score, mismatch_score, mismatch_cost, gap_open_score, gap_open_cost,
                                       gap_extension_score, gap_extension_cost)
    return _align_validated(good)


# --------------------------------------------------------------------------------
# The reference's DP building blocks, over its nested-list representation
# (list of rows of (level0, level1, level2) tuples).  They are thin shims over
# the same device kernels and exist so code written against globalign's
# internals (e.g. its own test-suite) keeps working.

def make_dp_array(seq_1, seq_2, costing_mat, max_cost, gap_open_cost):
    """(m+1) x (n+1) list with row 0 / column 0 set and None inside (globaligner.py:756-821)."""
    m, n = len(seq_1), len(seq_2)
    dp = [[None] * (n + 1) for _ in range(m + 1)]
    big = (max_cost + 1) * max(m, n)
    dp[0][0] = (0, 0, 0)
    if n >= 1:
        x = gap_open_cost + costing_mat["-"][seq_2[0]]
        dp[0][1] = (big, x, big)
        for j in range(2, n + 1):
            x += costing_mat["-"][seq_2[j - 1]]
            dp[0][j] = (big, x, big)
    else:
        return dp
    if m >= 1:
        y = gap_open_cost + costing_mat[seq_1[0]]["-"]
        dp[1][0] = (big, big, y)
        for i in range(2, m + 1):
            y += costing_mat[seq_1[i - 1]]["-"]
            dp[i][0] = (big, big, y)
    return dp


def _boundary_arrays(dp_array, m, n):
    row0 = np.array([dp_array[0][j] for j in range(n + 1)], dtype=np.int64).reshape(-1)
    col0 = np.array([dp_array[i][0] for i in range(m + 1)], dtype=np.int64).reshape(-1)
    if np.abs(np.concatenate([row0, col0])).max(initial=0) >= 2 ** 31:
        raise OverflowError("boundary values exceed the int32 range of the device path")
    return row0.astype(np.int32), col0.astype(np.int32)


def dp_array_forward(dp_array, seq_1, seq_2, costing_mat, gap_open_cost):
    """Fill dp_array[i][j] for i, j >= 1 in place from its row 0 / column 0 (globaligner.py:366-392)."""
    m, n = len(seq_1), len(seq_2)
    if m == 0 or n == 0:
        return None
    tables = _native.CostTables(costing_mat, gap_open_cost)
    row0, col0 = _boundary_arrays(dp_array, m, n)
    eng = _native.default_engine()
    eng.load(tables.codes(seq_1), tables.codes(seq_2), tables, row0=row0, col0=col0)
    _, full = eng.fill(full=True)
    for i in range(1, m + 1):
        row = dp_array[i]
        fi = full[i]
        for j in range(1, n + 1):
            row[j] = (int(fi[j, 0]), int(fi[j, 1]), int(fi[j, 2]))
    return None


def dp_array_backward(dp_array, seq_1, seq_2, costing_mat, gap_open_cost):
    """Traceback of a filled dp_array -> (seq_1_aligned, middle_part, seq_2_aligned, cost) (globaligner.py:395-593).

    Like the reference it walks the CALLER's cells (edited or hand-made ones included): the whole
    array goes to the device, a kernel derives every cell's traceback word from its (M, X, Y), and
    the walk kernel follows them.  Every interior cell must hold a triple (the reference would
    raise TypeError on a None it walks into; here any None raises it)."""
    m, n = len(seq_1), len(seq_2)
    tables = _native.CostTables(costing_mat, gap_open_cost)
    try:
        cells = np.array([[tuple(c) for c in row] for row in dp_array], dtype=np.int64)
    except TypeError:
        raise TypeError("'NoneType' object is not subscriptable") from None
    if cells.shape != (m + 1, n + 1, 3):
        raise IndexError("list index out of range")
    if np.abs(cells).max(initial=0) >= 2 ** 31:
        raise OverflowError("dp_array values exceed the int32 range of the device path")
    cells = cells.astype(np.int32)
    row0, col0 = cells[0].reshape(-1).copy(), cells[:, 0].reshape(-1).copy()
    eng = _native.default_engine()
    eng.load(tables.codes(seq_1), tables.codes(seq_2), tables, row0=row0, col0=col0)
    cost = eng.set_cells(cells)
    (a, mid, b), status, mt = eng.traceback(_mt_words(), seq_1, seq_2)
    _set_mt_words(mt)
    if status == _native.GA_TB_INDEX_ERROR:
        raise IndexError("string index out of range")
    return a, mid, b, cost


def _cli_version():
    """version('globalign') as the reference's --version prints it (globaligner.py:31-36): the installed
    globalign distribution's version, this package's own when globalign itself is not installed."""
    from importlib.metadata import PackageNotFoundError, version
    try:
        return version("globalign")
    except PackageNotFoundError:
        return __version__


def main(argv=None):
    """The `globaligner` command line (globaligner.py:23-129)."""
    parser = argparse.ArgumentParser(description="Perform optimal global alignment of two nucleotide or amino acid "
                                                 "sequences.")
    parser.add_argument("--version", action="version", version=_cli_version(), help="Prints the version and exits.")
    parser.add_argument("-i", "--input_fasta", required=False,
                        help="FASTA file with the two sequences to align (only the first 2 records are used).")
    parser.add_argument("-o", "--output", required=False,
                        help="Output file for the alignment; stdout when omitted.")
    parser.add_argument("--seq_1", required=False, help="First sequence to align.")
    parser.add_argument("--seq_2", required=False, help="Second sequence to align.")
    parser.add_argument("--scoring_mat_name", required=False, choices=["BLOSUM50", "BLOSUM62"],
                        help="Either 'BLOSUM50' or 'BLOSUM62'.")
    parser.add_argument("--scoring_mat_path", required=False, help="Path to a custom scoring matrix file.")
    parser.add_argument("--match_score", required=False, help="Score for a match (default 2).")
    parser.add_argument("--mismatch_score", required=False, help="Score for a mismatch (default -3).")
    parser.add_argument("--mismatch_cost", required=False, help="Cost for a mismatch (default 5).")
    parser.add_argument("--gap_open_score", required=False, help="Score for opening a run of gaps (default -4).")
    parser.add_argument("--gap_open_cost", required=False, help="Cost for opening a run of gaps (default 4).")
    parser.add_argument("--gap_extension_score", required=False, help="Score per gap (default -2).")
    parser.add_argument("--gap_extension_cost", required=False, help="Cost per gap (default 3).")
    args = parser.parse_args(argv)
    results = find_global_alignment(**vars(args))
    results.write()
    return None


if __name__ == "__main__":
    sys.exit(main())
