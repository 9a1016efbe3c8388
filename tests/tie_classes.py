"""Tie-rich cost tables, the census of the decision classes a traceback walk enters, and the case lists the tie-class
tests run (tests/test_tie_classes_cpu.py on the CPU, tests/test_gpu_tie_classes.py on every GPU decoder).

A walked cell is entered at a level L (0 diagonal, 1 gap in seq_1, 2 gap in seq_2).  Its triple (M, X, Y), with the
gap open cost o added to the two values that would open or switch a gap at levels 1 and 2, has a non-empty argmin set
S; (L, S, a_i == b_j) selects the bit field of the tie-break entry that names the next level: 3 x 7 x 2 = 42 SET
classes.  The LUT decoders index by a finer key: whether M is a minimum of the raw triple, and the differences
X - min and Y - min each classed against o as "0" (== 0), "lt" (0 < d < o), "eq" (== o) or "gt" (> o), at least one of
the three at zero: 23 combinations, times 2 for the match, times 3 levels: 138 JOINT classes.

Everything here is deterministic and imports without pytest.  A case is (family, table seed, o, m, n, sequence seed):

  T  tie-rich: sub entries drawn from {0, 1, 2o+1, 2o+2, 2o+2, 2o+3, 2o+4}, every gap cost 1 or 2.
  J  small random: sub entries uniform in 0..2o+4, every gap cost 1 or 2 (fields strictly between 0 and o).
  A  admissible to the int8 query profile at a large o (the lane fill and the recompute walk take only
     |sub - gap_v - gap_h| <= 127): gap costs g or g + 1 with g one of 1, 2, 30, 60, 63, sub either 0 or 1 or
     sub' = sub - gap_v - gap_h from {127, 127, 126, 125, 124, 64, 0, 1, 2}.

scaled(problem, k) multiplies every cost and o by k: every comparison keeps its outcome, so strings, random state and
census are those of the base case while o moves across the word-width switches (one byte: o + 1 < 8, two: o < 127).
"""
import collections
import random

from tests import general_costs as gc

LETTERS = gc.LETTERS
LEVELS = (0, 1, 2)
SETS = (1, 2, 3, 4, 5, 6, 7)                       # bit 0 M, bit 1 X, bit 2 Y
FIELD = ("0", "lt", "eq", "gt")
JOINT = tuple((zm, cx, cy) for zm in (1, 0) for cx in range(4) for cy in range(4) if zm or cx == 0 or cy == 0)
assert len(JOINT) == 23
SET_CLASSES = tuple((L, S, am) for L in LEVELS for S in SETS for am in (1, 0))
JOINT_CLASSES = tuple((L, J, am) for L in LEVELS for J in JOINT for am in (1, 0))
TIE_CLASSES = tuple(c for c in SET_CLASSES if c[1] & (c[1] - 1))
SINGLE_CLASSES = tuple(c for c in SET_CLASSES if not c[1] & (c[1] - 1))
assert (len(SET_CLASSES), len(JOINT_CLASSES), len(TIE_CLASSES), len(SINGLE_CLASSES)) == (42, 138, 24, 18)
MIN_TIE, MIN_SINGLE, MIN_JOINT = 8, 2, 1


def set_name(c):
    L, S, am = c
    return f"L{L}:{''.join(ch for k, ch in enumerate('MXY') if S >> k & 1)}:{'match' if am else 'mismatch'}"


def joint_name(c):
    L, (zm, cx, cy), am = c
    return f"L{L}:{'M' if zm else 'm'}/X{FIELD[cx]}/Y{FIELD[cy]}:{'match' if am else 'mismatch'}"


def tb_word_bytes(o):
    """ga_check.h tb_word_bytes, restated."""
    return 1 if o + 1 < 8 else 2 if o + 1 < 128 else 4


# ---------------------------------------------------------------- tables and cases
def _table(family, tseed, o):
    rng = random.Random((ord(family) << 40) ^ (tseed << 12) ^ o)
    if family == "A":
        g = rng.choice([1, 2, 30, 60, 63, 63])
        gh = [g + rng.randint(0, 1) for _ in range(4)]
        gv = [g + (rng.randint(0, 1) if g != 63 else 0) for _ in range(4)]
        pool = [None, None, 127, 127, 126, 125, 124, 64, 0, 1, 2]
        sub = [[0] * 4 for _ in range(4)]
        for x in range(4):
            for y in range(4):
                p = rng.choice(pool)
                sub[x][y] = rng.randint(0, 1) if p is None else p + gv[x] + gh[y]
        cmat = gc._dict(sub, gh, gv)
        assert gc.profile_bytes(cmat) == 1
        return cmat
    gh, gv = [rng.randint(1, 2) for _ in range(4)], [rng.randint(1, 2) for _ in range(4)]
    if family == "T":
        pool = [0, 1, 2 * o + 1, 2 * o + 2, 2 * o + 2, 2 * o + 3, 2 * o + 4]
        sub = [[rng.choice(pool) for _ in range(4)] for _ in range(4)]
    elif family == "J":
        sub = [[rng.randint(0, 2 * o + 4) for _ in range(4)] for _ in range(4)]
    else:
        raise ValueError(family)
    return gc._dict(sub, gh, gv)


def problem(case):
    """(costing dict, seq_1, seq_2, gap open cost) of a case, as tests/gpu_parity.py takes it."""
    family, tseed, o, m, n, sseed = case
    base = ((ord(family) * 1_000_003 + tseed) * 1_000_003 + sseed * 7919 + o) & gc.M64
    return _table(family, tseed, o), gc.splitmix_seq(m, base), gc.splitmix_seq(n, base + 1), o


def scaled(prob, k):
    """Every cost and the gap open cost times k."""
    cmat, s1, s2, o = prob
    return {x: {y: v * k for y, v in row.items()} for x, row in cmat.items()}, s1, s2, o * k


def admissible(prob):
    """Whether the int8 query profile takes the problem's table (the lane fill, the recompute walk)."""
    return gc.profile_bytes(prob[0]) == 1


# ---------------------------------------------------------------- census
def _cls(d, o):
    return 0 if d == 0 else 1 if d < o else 2 if d == o else 3


def census(prob, seed):
    """Two Counters over the cells the oracle's walk from random.seed(seed) enters, keyed (L, S, match) and
    (L, (M is a minimum, class of X - min, class of Y - min), match), from the oracle's full cell values and its
    alignment strings; the walk is followed up to its first cell on row 0 or column 0.
    -> (set counter, joint counter, (cost, strings, status, mt words))"""
    from tests import gpu_parity as gp
    cmat, s1, s2, o = prob
    dp = gp.full_reference(prob)[0]
    ref = gp.ref_chain(prob, seed)[0]
    a, _, b = ref[1]
    sets, joint = collections.Counter(), collections.Counter()
    i, j, L = len(s1), len(s2), 0
    for p in range(len(a) - 1, -1, -1):
        if i == 0 or j == 0:
            break
        v = [int(x) for x in dp[i, j]]
        w = (v[0] + (o if L else 0), v[1] + (o if L == 2 else 0), v[2] + (o if L == 1 else 0))
        S = sum(1 << k for k in range(3) if w[k] == min(w))
        am = int(s1[i - 1] == s2[j - 1])
        mn = min(v)
        # the move the oracle took must be one of the minima this census decoded for the cell
        move = 1 if a[p] == "-" else 2 if b[p] == "-" else 0
        assert S >> move & 1, (i, j, L, S, move)
        sets[(L, S, am)] += 1
        joint[(L, (int(v[0] == mn), _cls(v[1] - mn, o), _cls(v[2] - mn, o)), am)] += 1
        if a[p] == "-":
            j, L = j - 1, 1
        elif b[p] == "-":
            i, L = i - 1, 2
        else:
            i, j, L = i - 1, j - 1, 0
    return sets, joint, ref


def case_seed(case):
    """The random seed a case's walks start from."""
    return (case[1] * 131 + case[5]) & 0x7FFFFFFF


def census_of(cases):
    """Summed census of a case list."""
    sets, joint = collections.Counter(), collections.Counter()
    for c in cases:
        s, jn, _ = census(problem(c), case_seed(c))
        sets.update(s)
        joint.update(jn)
    return sets, joint


def deficit(sets, joint, targets=None):
    """What a census still lacks of the three conditions over the target classes (None: all) -> {class: missing}."""
    tset, tjoint = targets if targets else (SET_CLASSES, JOINT_CLASSES)
    out = {}
    for c in tset:
        need = MIN_TIE if c[1] & (c[1] - 1) else MIN_SINGLE
        if sets[c] < need:
            out[("set",) + c] = need - sets[c]
    for c in tjoint:
        if joint[c] < MIN_JOINT:
            out[("joint",) + c] = MIN_JOINT - joint[c]
    return out


# ---------------------------------------------------------------- the committed case lists (printed by search() below)
# BASE: greedy cover of the three conditions over all 42 set classes and all 138 joint classes; none is left out.
BASE = [
    ('J', 1, 2, 500, 600, 11), ('T', 6, 1, 500, 600, 17), ('T', 1, 2, 500, 600, 17), ('T', 0, 1, 500, 600, 15),
    ('T', 6, 1, 500, 600, 18), ('T', 3, 2, 500, 600, 15), ('T', 1, 1, 500, 600, 19), ('T', 3, 1, 500, 600, 9),
    ('J', 5, 2, 500, 600, 11), ('T', 6, 2, 500, 600, 16), ('T', 0, 1, 500, 600, 5), ('T', 0, 1, 500, 600, 6),
    ('T', 2, 1, 500, 600, 16), ('T', 1, 1, 500, 600, 7), ('T', 2, 1, 500, 600, 1), ('T', 7, 3, 500, 600, 0),
    ('T', 0, 1, 500, 600, 0), ('T', 7, 2, 500, 600, 13), ('J', 1, 2, 500, 600, 3), ('T', 1, 1, 500, 600, 1),
    ('T', 4, 1, 500, 600, 12), ('T', 5, 1, 500, 600, 14), ('T', 5, 1, 500, 600, 19), ('T', 0, 2, 500, 600, 0),
    ('T', 0, 2, 500, 600, 2), ('T', 7, 2, 500, 600, 2), ('T', 4, 3, 500, 600, 12), ('T', 4, 3, 500, 600, 17),
    ('T', 6, 3, 500, 600, 7),
]
# ZERO: o = 0, one-byte words only; all three levels share one set there, so a joint class is its set class: the list
# enters each of the 42 at least once (no count is asked of it).
ZERO = [
    ('T', 3, 0, 500, 600, 6), ('T', 3, 0, 500, 600, 7), ('T', 0, 0, 500, 600, 1), ('T', 3, 0, 500, 600, 2),
    ('T', 2, 0, 500, 600, 0), ('T', 0, 0, 500, 600, 5), ('T', 3, 0, 500, 600, 8), ('T', 5, 0, 500, 600, 7),
]
# INT8_LARGE: four-byte words under an int8 query profile (o = 127 and 130).  A mismatch that ties with a gap in each
# sequence costs 2 o + gap_v + gap_h, i.e. sub' = 2 o > 127: the tie mechanism of family T is out of the profile's
# reach once o >= 64, and the three-way ties that rest on it become rare.  The search still enters every class; the
# four below stay under eight visits in 40 cases (INT8_LARGE_SHORT: the class and its count in this list).
INT8_LARGE = [
    ('A', 56, 127, 500, 600, 34), ('A', 37, 130, 500, 600, 26), ('A', 4, 127, 500, 600, 17),
    ('A', 26, 130, 500, 600, 37), ('A', 39, 127, 500, 600, 27), ('A', 1, 130, 500, 600, 2),
    ('A', 6, 127, 500, 600, 20), ('A', 22, 127, 500, 600, 12), ('A', 22, 127, 500, 600, 18),
    ('A', 26, 130, 500, 600, 0), ('A', 26, 130, 500, 600, 29), ('A', 28, 127, 500, 600, 12),
    ('A', 1, 130, 500, 600, 5), ('A', 1, 130, 500, 600, 32), ('A', 16, 127, 500, 600, 10),
    ('A', 26, 130, 500, 600, 39), ('A', 39, 127, 500, 600, 5), ('A', 39, 127, 500, 600, 8),
    ('A', 44, 127, 500, 600, 14), ('A', 47, 130, 500, 600, 25), ('A', 56, 127, 500, 600, 36),
    ('A', 1, 130, 500, 600, 1), ('A', 22, 127, 500, 600, 2), ('A', 26, 130, 500, 600, 7),
    ('A', 32, 127, 500, 600, 6), ('A', 32, 127, 500, 600, 15), ('A', 32, 127, 500, 600, 27),
    ('A', 37, 130, 500, 600, 32), ('A', 38, 127, 500, 600, 25), ('A', 39, 127, 500, 600, 12),
    ('A', 44, 127, 500, 600, 15), ('A', 47, 130, 500, 600, 33), ('A', 1, 130, 500, 600, 10),
    ('A', 1, 130, 500, 600, 14), ('A', 1, 130, 500, 600, 16), ('A', 1, 130, 500, 600, 21),
    ('A', 1, 130, 500, 600, 22), ('A', 1, 130, 500, 600, 30), ('A', 1, 130, 500, 600, 36),
    ('A', 1, 130, 500, 600, 38),
]
INT8_LARGE_SHORT = {(1, 7, 1): 1, (1, 7, 0): 6, (2, 7, 1): 1, (2, 7, 0): 6}
# a few family-A cases at o = 126, the last two-byte gap open cost, for the int8 paths (on top of their two-byte list)
INT8_126 = [("A", t, 126, 500, 600, s) for t, s in ((56, 34), (4, 17), (39, 27), (22, 12), (32, 6), (44, 14))]

# scale factors by base o and word width: o k lands on 6 | 7 (8, 9) and 126 | 127 (128, 129), both sides of each switch
FACTORS = {1: {1: (1, 6), 2: (7, 126), 4: (127,)}, 2: {1: (1, 3), 2: (4, 63), 4: (64,)}, 3: {1: (1, 2), 2: (3, 42), 4: (43,)}}
WIDTHS = (1, 2, 4)


def width_cases(width, int8=False):
    """[(case, k)] of a word width: BASE with the width's factors taken in turn (the census does not depend on k), at
    width 1 ZERO as well.  int8: the list of the paths that take an int8 query profile only -- two-byte words keep
    the lower factor (o 7..9; the upper one leaves the profile) and add INT8_126, four-byte words run INT8_LARGE."""
    if int8 and width == 4:
        return [(c, 1) for c in INT8_LARGE]
    out = []
    for q, c in enumerate(BASE):
        ks = FACTORS[c[2]][width]
        out.append((c, ks[0] if int8 and width == 2 else ks[q % len(ks)]))
    if width == 1:
        out += [(c, 1) for c in ZERO]
    if int8 and width == 2:
        out += [(c, 1) for c in INT8_126]
    return out


def targets(width, int8=False):
    """(set classes, joint classes) a width's list must cover under the three conditions, and {set class: count} of
    the named exceptions that stay under their count."""
    if int8 and width == 4:
        return (SET_CLASSES, JOINT_CLASSES), dict(INT8_LARGE_SHORT)
    return (SET_CLASSES, JOINT_CLASSES), {}


def base_part(pairs):
    """The cases of a width list that the conditions are counted over (o >= 1, without the o = 126 extras)."""
    return [c for c, _ in pairs if c[2] != 0 and c not in INT8_126]


def scaled_problem(case, k):
    p = problem(case)
    return p if k == 1 else scaled(p, k)


# ---------------------------------------------------------------- the search (run by hand; its output is pasted above)
def candidates(families, opens, tseeds, sseeds, m=500, n=600):
    return [(f, t, o, m, n, s) for f in families for o in opens for t in tseeds for s in sseeds]


def greedy_cover(cands, limit=40, verbose=False):
    """Greedy cover: repeatedly the candidate that removes most of what the three conditions still lack.
    -> (cases, union of set classes reached by all candidates, union of joint classes reached)"""
    cens = {}
    for c in cands:
        s, jn, _ = census(problem(c), case_seed(c))
        cens[c] = (s, jn)
    reach_s = set().union(*[set(s) for s, _ in cens.values()])
    reach_j = set().union(*[set(jn) for _, jn in cens.values()])
    targets = ([c for c in SET_CLASSES if c in reach_s], [c for c in JOINT_CLASSES if c in reach_j])
    chosen, sets, joint = [], collections.Counter(), collections.Counter()
    lack = deficit(sets, joint, targets)
    while lack and len(chosen) < limit:
        def gain(c):
            s, jn = cens[c]
            return sum(min(v, (s if k[0] == "set" else jn)[k[1:]]) for k, v in lack.items())
        best = max((c for c in cands if c not in chosen), key=gain)
        if gain(best) == 0:
            break
        chosen.append(best)
        sets.update(cens[best][0])
        joint.update(cens[best][1])
        lack = deficit(sets, joint, targets)
        if verbose:
            print(len(chosen), best, "lack", sum(lack.values()))
    return chosen, reach_s, reach_j, lack


def search():
    """Prints the committed lists: BASE (families T and J, o 1..3), ZERO (family T at o = 0) and INT8_LARGE (family A
    at o = 127 and 130, in two stages: every table with a few sequence pairs, then the tables of the first stage's
    pick with many)."""
    base = candidates("T", (1, 2, 3), range(8), range(20)) + candidates("J", (2, 3), range(6), range(12))
    for name, cands, limit in (("BASE", base, 40), ("ZERO", candidates("T", (0,), range(8), range(12)), 8)):
        chosen, rs, rj, lack = greedy_cover(cands, limit)
        print(name, "=", chosen)
        print("#", len(chosen), "cases; set classes reached", len(rs), "joint", len(rj), "lack", lack)
    first, _, _, _ = greedy_cover(candidates("A", (127, 130), range(60), range(6)), 40)
    tabs = sorted({(c[1], c[2]) for c in first})
    chosen, rs, rj, lack = greedy_cover([("A", t, o, 500, 600, s) for t, o in tabs for s in range(40)], 40)
    print("INT8_LARGE =", chosen)
    print("#", len(chosen), "cases; set classes reached", len(rs), "joint", len(rj))
    print("# lack", {(set_name(k[1:]) if k[0] == "set" else joint_name(k[1:])): v for k, v in lack.items()})
    print("# never reached", [set_name(c) for c in SET_CLASSES if c not in rs],
          [joint_name(c) for c in JOINT_CLASSES if c not in rj])


def existing_census(max_cells=8_000_000):
    """Prints, for the walk case lists the suite had before this module (tests/general_costs.py ROW_WALK, lane walks,
    RC, BANDED; the DNA inputs of tests/test_gpu_rc.py) and for this module's lists, the set and joint classes their
    walks enter, by traceback word width (DESIGN.md 2 holds the output; nothing asserts on it)."""
    from oracle import transform
    from tests.conftest import splitmix_seq

    def gprob(case):
        s1, s2 = gc.sequences(case)
        return gc.table(case[0], case[1]), s1, s2, case[4]

    def dna(m, n, sa, sb, seed, o=5):
        kw = dict(match_score=2, mismatch_score=-3, gap_open_score=-o, gap_extension_score=-1)
        s1, s2 = splitmix_seq(m, sa, "dna"), splitmix_seq(n, sb, "dna")
        a1, a2, _, cmat, _, goc = transform.settings(dict(kw, seq_1=s1, seq_2=s2))
        return (cmat, a1, a2, goc), seed

    lists = {
        "general_costs.ROW_WALK": [(gprob(c), c[2] ^ c[3]) for c in gc.ROW_WALK],
        "general_costs lane walks": [(gprob(c), td + c[2]) for td in (1, 2, 4) for c in gc.lane_walk_cases(td)],
        "general_costs.RC": [(gprob(c), c[2] + c[4]) for c, _, _ in gc.RC],
        "general_costs.BANDED": [(gprob(c), c[3] ^ b) for c, b in gc.BANDED],
        "test_gpu_rc DNA inputs": [dna(m, n, 11, 12, m + n) for m, n in ((256, 256), (300, 500), (1000, 1300), (777, 2049),
                                                                      (2049, 3000), (5000, 300), (300, 5000))] +
                                  [dna(1500, 1700, 51, 52, o, o) for o in (7, 130)],
        "tie_classes, any profile": [(scaled_problem(c, k), case_seed(c)) for w in WIDTHS for c, k in width_cases(w)],
        "tie_classes, int8 profile": [(scaled_problem(c, k), case_seed(c)) for w in WIDTHS
                                      for c, k in width_cases(w, True)],
    }
    print("| case list | width | cases | set classes of 42 | tie classes with >= 8 visits of 24 | joint classes of 138 |")
    print("|---|---|---|---|---|---|")
    for name, items in lists.items():
        for w in WIDTHS:
            sets, joint, count = collections.Counter(), collections.Counter(), 0
            for prob, seed in items:
                if tb_word_bytes(prob[3]) != w or (len(prob[1]) + 1) * (len(prob[2]) + 1) > max_cells:
                    continue
                s, jn, _ = census(prob, seed)
                sets.update(s)
                joint.update(jn)
                count += 1
            if count:
                ties = sum(sets[c] >= MIN_TIE for c in TIE_CLASSES)
                print(f"| {name} | {w} | {count} | {len(sets)} | {ties} | {len(joint)} |")


if __name__ == "__main__":
    search()
