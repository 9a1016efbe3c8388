"""Planted alignment paths, the census of where a traceback walk goes, and the case lists the path-geometry tests run
(tests/test_path_geometry_cpu.py on the CPU, tests/test_gpu_path_geometry.py on every GPU walker).

tests/tie_classes.py covers what a walked cell can decide; this module covers where the path goes.  Every walker has
control flow that depends on the path's geometry: walk_body (ga_walk.h) runs check-free 16-step iterations only while
min(i, j) > 16 (24 for the next one) and only inside tiles verified with margins 19 and 27, over a 4 x 4 torus of
64 x 64 tiles whose loaders leave out the block's far off-diagonal tiles; levels leave through a ring of four
512-dispatch blocks; the batch walker reads an 8 x 8 window clamped at row 1 and column 1; banded_align
(ga_align_host.cpp) refills each band up to the walk's entry column and hands the walk on at every band top; the
recompute walk ranks candidate blocks at most 7 stripes left and 31 block rows up; slabs hand the walk on at their
local column 0.  Of the suite's earlier walk inputs only one list has a gap run across more than four tile seams
away from the matrix edges, and none plants where a run starts or ends, where the walk arrives, or how many
dispatches it takes (existing_census()).

Everything here is deterministic and imports without pytest.  A case is (costs, segments, seed):

  costs     ("dna", o): the everyday DNA table (match 0, mismatch 5, every gap 2: scores 2 / -3 / -1), int8 profile;
            ("gap", o): "gaps only", match 0, every gap 1, mismatch 2 + 2 o + 2 (dearer than two gaps and two gap
            opens): letters that differ are never aligned.  Its sub' is 2 o + 2: int8 profile up to o = 62.
            ("gap8", o): match 0, every gap 1, mismatch 127 (sub' = 125, the int8 profile at any o): a Z corner of
            d x d letters goes by gaps only once d mismatches cost more than the 2 d gaps and two gap opens,
            125 d > 2 o -- at o = 127 from d = 3 on.  The int8 paths' four-byte lists take it in place of "gap".
  segments  a tuple of ("D", k)  k identical letters in both sequences,
                       ("N", k)  the same with about 6 % substitutions (a few ties),
                       ("H", k)  k letters in seq_2 only,
                       ("V", k)  k letters in seq_1 only,
                       ("Z", k1, k2)  k1 letters over {A, C} in seq_1 and k2 over {G, T} in seq_2: gaps only under
                                 the "gap" table; at o > 0 one run of each kind, their order chosen by the
                                 tie-break, at o = 0 a random lattice walk.
  letters   gc.splitmix_seq draws, seeded by (seed, segment index).

The lists are kept by kind ("dna", "gap" or "gap0") and take their gap open cost from the traceback word width asked
for (OPENS): the geometry of a planted path does not depend on o, and the census of every width's list is taken at
that width's o (tests/test_path_geometry_cpu.py).
"""
import collections
import random

from tests import general_costs as gc

TILE = 64
CELL_CAP, SIDE_CAP, COUNT_CAP = 1_500_000, 2600, 48
BATCH_CELL_CAP = 1 << 20                     # ga_batch.h kDefaultAlignMaxCells
FROWS = 16                                   # ga_device.h ga::FROWS: the band remainder rule of banded_align
BAND_ROWS = (16, 64)
WIDTHS = (1, 2, 4)
# gap open costs by table kind and traceback word width (one byte: o + 1 < 8, two: o + 1 < 128), taken in turn
OPENS = {"dna": {1: (5,), 2: (7, 8, 9), 4: (127, 130)}, "gap": {1: (3,), 2: (8,), 4: (127,)}, "gap0": {1: (0,)}}
DIST_CLASSES = ((1, 16), (17, 24), (25, 63), (64, 255), (256, 1 << 30))


def tb_word_bytes(o):
    """ga_check.h tb_word_bytes, restated."""
    return 1 if o + 1 < 8 else 2 if o + 1 < 128 else 4


def slab_bounds(n, world=3, align=512):
    """globalign_amd.distributed.slab_bounds, restated (this module imports without the package)."""
    edges = [0]
    for k in range(1, world):
        e = int(round(n * k / world / align)) * align
        e = min(max(e, edges[-1] + 1), n - (world - k))
        edges.append(e)
    edges.append(n)
    return edges


# ---------------------------------------------------------------- problems
def cost_table(kind, o):
    if kind == "dna":
        sub, gap = [[0 if x == y else 5 for y in range(4)] for x in range(4)], 2
    elif kind == "gap":
        sub, gap = [[0 if x == y else 2 + 2 * o + 2 for y in range(4)] for x in range(4)], 1
    elif kind == "gap8":
        sub, gap = [[0 if x == y else 127 for y in range(4)] for x in range(4)], 1
    else:
        raise ValueError(kind)
    return gc._dict(sub, [gap] * 4, [gap] * 4)


def _letters(k, seed, q, salt=0):
    return gc.splitmix_seq(k, ((seed * 1_000_003 + q) * 1_000_003 + salt * 7919 + 12345) & gc.M64)


def sequences(segments, seed):
    s1, s2 = [], []
    for q, seg in enumerate(segments):
        kind, k = seg[0], seg[1]
        if kind == "D":
            x = _letters(k, seed, q)
            s1.append(x)
            s2.append(x)
        elif kind == "N":
            x, f1, f2 = _letters(k, seed, q), _letters(k, seed, q, 1), _letters(k, seed, q, 2)
            y = "".join("ACGT"[("ACGT".index(c) + 1) % 4] if f1[p] == "A" and f2[p] == "A" else c
                        for p, c in enumerate(x))
            s1.append(x)
            s2.append(y)
        elif kind == "H":
            s2.append(_letters(k, seed, q))
        elif kind == "V":
            s1.append(_letters(k, seed, q))
        elif kind == "Z":
            s1.append("".join("ACAC"["ACGT".index(c)] for c in _letters(k, seed, q)))
            s2.append("".join("GTGT"["ACGT".index(c)] for c in _letters(seg[2], seed, q, 1)))
        else:
            raise ValueError(seg)
    return "".join(s1), "".join(s2)


def problem(case):
    """(costing dict, seq_1, seq_2, gap open cost) of a case, as tests/gpu_parity.py takes it."""
    (kind, o), segments, seed = case
    s1, s2 = sequences(segments, seed)
    return cost_table(kind, o), s1, s2, o


def shape(case):
    _, segments, _ = case
    m = sum(s[1] for s in segments if s[0] in "DNVZ")
    n = sum(s[2] if s[0] == "Z" else s[1] for s in segments if s[0] in "DNHZ")
    return m, n


def case_seed(case):
    """The random seed a case's walks start from."""
    return (case[2] * 131 + len(case[1])) & 0x7FFFFFFF


def admissible(prob):
    """Whether the int8 query profile takes the problem's table (the lane fill, the recompute walk)."""
    return gc.profile_bytes(prob[0]) == 1


# ---------------------------------------------------------------- census
Census = collections.namedtuple("Census", "steps end D runs phases corners arrival corridors depths reach ref")


def _seams(lo, hi, period):
    """Seams of `period` a move sequence crosses going from coordinate hi down to lo (cells hi .. lo, 1-based:
    coordinates c and c - 1 lie in different tiles when c - 1 is a positive multiple of the period)."""
    return sum(1 for c in range(lo + 1, hi + 1) if (c - 1) % period == 0 and c - 1 > 0)


def census(prob, seed, rows=TILE, cols=TILE):
    """The geometry of the oracle's walk from random.seed(seed), followed from (m, n) to its first cell on row 0 or
    column 0 (tie_classes.census's convention); every move is asserted to be one of the cell's minima, from the
    oracle's full cell values.  A dispatch is one walked cell: (i, j, entering level, move), move 0 diagonal, 1 a gap
    in seq_1 (j falls), 2 a gap in seq_2 (i falls).

      steps      the dispatches; end: the edge cell reached; D = len(steps), what the kernels count
      runs       maximal gap runs: (level, length, first cell (where the first gap move is made), last cell (where
                 the last one arrives), seams crossed at the axis' period, index of the first dispatch)
      phases     Counter of (level, "start" | "end", "first" | "last"): the run's first / last cell is the first /
                 last of its tile along the run's axis
      corners    [(dispatch index, after a gap move, before a gap move)] of diagonal moves from (rows a + 1, cols b + 1)
      arrival    (edge "row" | "col" | "corner", level of the last move, the other coordinate)
      corridors  {("row" | "col", r): (longest stretch of consecutive dispatches with i <= r / j <= r, seams crossed
                 along it)} for r in (7, 16, 24)
      depths     {("row" | "col", p): (longest stretch of consecutive dispatches at i == p / j == p, seams)}, p <= 25
      reach      largest tile distance from the start tile's diagonal
    """
    from tests import gpu_parity as gp
    cmat, s1, s2, o = prob
    dp = gp.full_reference(prob)[0]
    ref = gp.ref_chain(prob, seed)[0]
    a, _, b = ref[1]
    steps = []
    i, j, L = len(s1), len(s2), 0
    for p in range(len(a) - 1, -1, -1):
        if i == 0 or j == 0:
            break
        v = [int(x) for x in dp[i, j]]
        w = (v[0] + (o if L else 0), v[1] + (o if L == 2 else 0), v[2] + (o if L == 1 else 0))
        move = 1 if a[p] == "-" else 2 if b[p] == "-" else 0
        assert w[move] == min(w), (i, j, L, w, move)
        steps.append((i, j, L, move))
        if move == 1:
            j, L = j - 1, 1
        elif move == 2:
            i, L = i - 1, 2
        else:
            i, j, L = i - 1, j - 1, 0
    assert i == 0 or j == 0
    end, D = (i, j), len(steps)

    def cell(d):
        return steps[d][:2] if d < D else end

    runs, phases = [], collections.Counter()
    d = 0
    while d < D:
        mv = steps[d][3]
        e = d
        while e + 1 < D and steps[e + 1][3] == mv:
            e += 1
        if mv:
            first, last = cell(d), cell(e + 1)
            ax = 1 if mv == 1 else 0
            runs.append((mv, e - d + 1, first, last, _seams(last[ax], first[ax], cols if mv == 1 else rows), d))
            per = cols if mv == 1 else rows
            for which, c in (("start", first[ax]), ("end", last[ax])):
                if c >= 1 and (c - 1) % per == 0:
                    phases[(mv, which, "first")] += 1
                if c >= 1 and (c - 1) % per == per - 1:
                    phases[(mv, which, "last")] += 1
        d = e + 1
    corners = [(d, d > 0 and steps[d - 1][3] != 0, d + 1 < D and steps[d + 1][3] != 0)
               for d, (ci, cj, _, mv) in enumerate(steps)
               if mv == 0 and ci > 1 and cj > 1 and (ci - 1) % rows == 0 and (cj - 1) % cols == 0]
    arrival = ("corner" if end == (0, 0) else "row" if end[0] == 0 else "col", steps[-1][3] if steps else 0,
               end[1] if end[0] == 0 else end[0])

    def stretch(ax, pred):
        best, d = (0, 0), 0
        while d < D:
            if not pred(steps[d][ax]):
                d += 1
                continue
            e = d
            while e + 1 < D and pred(steps[e + 1][ax]):
                e += 1
            other = 1 - ax
            cand = (e - d + 1, _seams(cell(e + 1)[other], steps[d][other], cols if other else rows))
            best = max(best, cand)
            d = e + 1
        return best

    corridors = {(name, r): stretch(ax, lambda c, r=r: c <= r) for ax, name in ((0, "row"), (1, "col"))
                 for r in (7, 16, 24)}
    depths = {(name, p): stretch(ax, lambda c, p=p: c == p) for ax, name in ((0, "row"), (1, "col"))
              for p in range(1, 26)}
    t0 = (len(s1) - 1) // rows - (len(s2) - 1) // cols
    reach = max([abs((ci - 1) // rows - (cj - 1) // cols - t0) for ci, cj, _, _ in steps] or [0])
    return Census(steps, end, D, runs, phases, corners, arrival, corridors, depths, reach, ref)


def band_count(m, Bh):
    """banded_align's bands [b Bh, b Bh + Bh) of rows, the last one absorbing a remainder of < 16 rows."""
    nb = (m + Bh - 1) // Bh
    if nb > 1 and m - (nb - 1) * Bh < FROWS:
        nb -= 1
    return nb


def band_crossings(cen, m, Bh):
    """-> ([(level of the move, column, D at the crossing)] of the moves that arrive on a band's top row b Bh,
    1 <= b < bands, at a column > 0; band the walk ends in; rows the last band holds beyond Bh)"""
    nb = band_count(m, Bh)
    out = []
    for d, (i, j, _, mv) in enumerate(cen.steps):
        if mv != 1 and (i - 1) % Bh == 0 and 1 <= (i - 1) // Bh < nb:
            col = j - 1 if mv == 0 else j
            if col > 0:
                out.append((mv, col, d + 1))
    ei = cen.end[0]
    return out, (min((ei - 1) // Bh, nb - 1) if ei > 0 else 0), m - (nb - 1) * Bh - Bh


def run_band_tops(run, m, Bh):
    """Band tops a level-2 run crosses (arrives on or passes)."""
    nb = band_count(m, Bh)
    return sum(1 for b in range(1, nb) if run[3][0] <= b * Bh < run[2][0])


def slab_crossings(cen, edges):
    """-> [(level of the move, row, D at the crossing, edge)] of the moves that arrive on an inner slab edge's column
    (the left slab's last column: local column 0 of the slab the walk leaves) at a row > 0."""
    out = []
    for d, (i, j, _, mv) in enumerate(cen.steps):
        if mv != 2 and (j - 1) in edges[1:-1]:
            row = i - 1 if mv == 0 else i
            if row > 0:
                out.append((mv, row, d + 1, j - 1))
    return out


# ---------------------------------------------------------------- conditions
def _dist_class(x):
    return next(k for k, (lo, hi) in enumerate(DIST_CLASSES) if lo <= x <= hi)


def classes(case, cen):
    """Counter of the condition classes a case's walk reaches (the class names are those of REQUIRED)."""
    m, n = shape(case)
    out = collections.Counter()
    for L, length, first, last, seams, d in cen.runs:
        interior = d >= 64 and min(last) >= 64
        if interior and seams >= 5:
            out[("W1", L)] += 1
        if interior and L == 1 and seams >= 9:
            out[("W1", "rc-stripes")] += 1
        if interior and L == 2 and seams >= 32:
            out[("W1", "rc-rows")] += 1
        if L == 1 and first[1] > 0:
            e = slab_bounds(n) if n >= 3 else None
            if e and first[1] > e[2] and last[1] < e[1]:
                out[("W8", "span-middle")] += 1
        if L == 2 and n >= 3:
            e = slab_bounds(n)
            if first[1] in (e[1] + 1, e[2] + 1):
                out[("W8", "v-first-column")] += 1
            if first[1] in (e[1], e[2]):
                out[("W8", "v-last-column")] += 1
        if L == 2:
            for Bh in BAND_ROWS:
                if run_band_tops((L, length, first, last), m, Bh) >= 3:
                    out[("W7", Bh, "v3")] += 1
    for k, v in cen.phases.items():
        out[("W2",) + k] += v
    out[("W3", "corner")] += len(cen.corners)
    out[("W3", "after-run")] += sum(1 for _, aft, _ in cen.corners if aft)
    out[("W3", "before-run")] += sum(1 for _, _, bef in cen.corners if bef)
    edge, L, other = cen.arrival
    out[("W4", "corner") if edge == "corner" else ("W4", edge, L, _dist_class(other))] += 1
    for (axis, p), (length, seams) in cen.depths.items():
        if p in (1, 7, 8, 16, 17, 24, 25) and length >= 300 and seams >= 4:
            out[("W5", axis, p)] += 1
    D = cen.D
    out[("W6", "mod16", D % 16)] += 1
    out[("W6", "mod512", D % 512)] += 1
    out[("W6", "mod4", D % 4)] += 1
    out[("W6", "D", D)] += 1
    if D >= 2049 and D % 16:
        out[("W6", "partial-after-wrap")] += 1
    for Bh in BAND_ROWS:
        cross, end_band, extra = band_crossings(cen, m, Bh)
        for L, col, d in cross:
            out[("W7", Bh, "cross", L)] += 1
            out[("W7", Bh, "entry", col)] += 1
            out[("W7", Bh, "dmod4", d % 4)] += 1
        if band_count(m, Bh) > 1:
            if edge == "col" and end_band >= 1:
                out[("W7", Bh, "col0-lower-band")] += 1
            if edge == "col" and other % Bh == 0 and other // Bh < band_count(m, Bh):
                out[("W7", Bh, "col0-on-band-top")] += 1
            if edge == "row":
                out[("W7", Bh, "row0-top-band")] += 1
            if 0 < extra < FROWS:
                out[("W7", Bh, "remainder")] += 1
    if n >= 3:
        e = slab_bounds(n)
        for L, row, d, _ in slab_crossings(cen, e):
            out[("W8", "cross", L)] += 1
            out[("W8", "dmod4", d % 4)] += 1
        if edge == "row" and e[1] < other <= e[2]:
            out[("W8", "row0-middle")] += 1
        if edge == "row" and other > e[2]:
            out[("W8", "row0-right")] += 1
    return +out


def _required():
    """{class: ("cases", k)  at least k different cases reach it | ("sum", k)  at least k visits over the list}"""
    req = {}
    two, once = ("cases", 2), ("cases", 1)
    # W1 runs beyond the 256 torus and the 4-tile block, into the tiles skip_corners leaves out (ga_walk.h loaders,
    # need_tile); rc-*: beyond the recompute walk's candidate window kSpanS = 7 stripes / kSpanI = 31 block rows
    req["W1"] = {("W1", 1): two, ("W1", 2): two}
    req["RC"] = {("W1", "rc-stripes"): once, ("W1", "rc-rows"): once}
    # W2 run phases against the tile seams (tile switches at a run's first / last move)
    req["W2"] = {("W2", L, w, ph): two for L in (1, 2) for w in ("start", "end") for ph in ("first", "last")}
    # W3 moves that cross a row seam and a column seam at once
    req["W3"] = {("W3", "corner"): ("sum", 4), ("W3", "after-run"): ("sum", 1), ("W3", "before-run"): ("sum", 1)}
    # W4 edge arrival: the CHECK groups, the iend / jend reasons, walk_tail's boundary run (ga_strings.h)
    req["W4"] = {("W4", e, L, k): two for e, Ls in (("row", (0, 2)), ("col", (0, 1))) for L in Ls
                 for k in range(len(DIST_CLASSES))}
    req["W4"][("W4", "corner")] = two
    # W5 corridors: thresholds 16 / 24, margins 19 / 27, vlo_i / vlo_j at tile row / column 0, the batch walker's
    # clamped 8 x 8 window
    req["W5"] = {("W5", ax, p): two for ax in ("row", "col") for p in (1, 7, 8, 16, 17, 24, 25)}
    # W6 dispatch counts: the level words (16 to a word, partial last word), the ring of four 512-dispatch blocks
    req["W6"] = {("W6", "mod16", r): two for r in (0, 1, 15)}
    req["W6"].update({("W6", "mod512", r): two for r in (0, 1, 511)})
    req["W6"].update({("W6", "mod4", r): two for r in range(4)})
    req["W6"].update({("W6", "D", 2048): once, ("W6", "D", 2049): once, ("W6", "partial-after-wrap"): once})
    # W7 banded_align: bd.nc = st.j, reason 6 at each band top, the loop's end at column 0 (also by a move that lands
    # on a band's top row and on column 0 at once: the walk tests row 0 first), the remainder rule
    req["W7"] = {}
    for Bh in BAND_ROWS:
        req["W7"].update({("W7", Bh, "v3"): two, ("W7", Bh, "cross", 0): ("sum", 8), ("W7", Bh, "cross", 2): ("sum", 8),
                          ("W7", Bh, "col0-lower-band"): two, ("W7", Bh, "col0-on-band-top"): two,
                          ("W7", Bh, "row0-top-band"): two,
                          ("W7", Bh, "remainder"): once})
        req["W7"].update({("W7", Bh, "entry", c): two for c in (1, 2, 63, 64, 65)})
        req["W7"].update({("W7", Bh, "dmod4", r): two for r in range(4)})
    # W8 slabs: reason 5 at local column 0 in either level, slabs that contribute a whole run or only the tail
    req["W8"] = {("W8", k): two for k in ("span-middle", "v-first-column", "v-last-column", "row0-middle", "row0-right")}
    req["W8"].update({("W8", "cross", L): two for L in (0, 1)})
    req["W8"].update({("W8", "dmod4", r): two for r in range(4)})
    return req


REQUIRED = _required()


def deficit(cases, groups, censuses=None):
    """What a case list lacks of the condition groups -> {class: missing}.  censuses: {case: Census} already made."""
    reach_cases, reach_sum = collections.Counter(), collections.Counter()
    for c in cases:
        cen = censuses[c] if censuses and c in censuses else census(problem(c), case_seed(c))
        for k, v in classes(c, cen).items():
            reach_cases[k] += 1
            reach_sum[k] += v
    out = {}
    for g in groups:
        for k, (how, need) in REQUIRED[g].items():
            have = reach_cases[k] if how == "cases" else reach_sum[k]
            if have < need:
                out[k] = need - have
    return out


# ---------------------------------------------------------------- the committed case lists (printed by search() below)
# (kind, segments, seed); the gap open cost comes from the word width (at_width)
LISTS = {
    # RUNS: W1, W2, W3
    'RUNS': [
        ('dna', (('D', 128), ('H', 384), ('D', 200)), 0), ('dna', (('D', 128), ('H', 384), ('D', 200)), 2),
        ('dna', (('D', 128), ('V', 384), ('D', 200)), 0), ('dna', (('D', 128), ('V', 384), ('D', 200)), 2),
        ('dna', (('D', 128), ('H', 384), ('N', 200)), 1), ('dna', (('D', 129), ('H', 384), ('D', 200)), 0),
        ('dna', (('D', 129), ('V', 384), ('D', 200)), 0), ('dna', (('D', 129), ('V', 384), ('D', 200)), 2),
    ],
    # RC_RUNS: the recompute list's W1 runs beyond kSpanS / kSpanI
    'RC_RUNS': [
        ('dna', (('D', 128), ('V', 2100), ('D', 200)), 0), ('dna', (('D', 300), ('H', 700), ('D', 300)), 0),
    ],
    # ARRIVE: W4 at one-byte words, then the Z corners of 16 x 16 letters that the int8 lists need at four-byte words
    # under "gap8"; the last two: o = 0 lattice walks, on top
    'ARRIVE': [
        ('dna', (('H', 1), ('D', 300)), 0), ('dna', (('V', 1), ('D', 300)), 0), ('dna', (('H', 1), ('D', 300)), 1),
        ('dna', (('V', 1), ('D', 300)), 1), ('gap', (('Z', 1, 1), ('D', 300)), 1),
        ('gap', (('Z', 1, 1), ('D', 300)), 2), ('gap', (('Z', 1, 1), ('D', 300)), 3),
        ('gap', (('Z', 1, 1), ('D', 300)), 4), ('dna', (('H', 17), ('D', 300)), 0),
        ('dna', (('V', 17), ('D', 300)), 0), ('dna', (('H', 17), ('D', 300)), 1), ('dna', (('V', 17), ('D', 300)), 1),
        ('gap', (('Z', 17, 17), ('D', 300)), 1), ('gap', (('Z', 17, 17), ('D', 300)), 2),
        ('gap', (('Z', 17, 17), ('D', 300)), 3), ('gap', (('Z', 17, 17), ('D', 300)), 4),
        ('dna', (('H', 25), ('D', 300)), 0), ('dna', (('V', 25), ('D', 300)), 0), ('dna', (('H', 25), ('D', 300)), 1),
        ('dna', (('V', 25), ('D', 300)), 1), ('gap', (('Z', 25, 25), ('D', 300)), 1),
        ('gap', (('Z', 25, 25), ('D', 300)), 2), ('gap', (('Z', 25, 25), ('D', 300)), 3),
        ('gap', (('Z', 25, 25), ('D', 300)), 4), ('dna', (('H', 64), ('D', 300)), 0),
        ('dna', (('V', 64), ('D', 300)), 0), ('dna', (('H', 64), ('D', 300)), 1), ('dna', (('V', 64), ('D', 300)), 1),
        ('gap', (('Z', 64, 64), ('D', 300)), 1), ('gap', (('Z', 64, 64), ('D', 300)), 2),
        ('gap', (('Z', 64, 64), ('D', 300)), 3), ('gap', (('Z', 64, 64), ('D', 300)), 4),
        ('dna', (('H', 256), ('D', 300)), 0), ('dna', (('V', 256), ('D', 300)), 0),
        ('dna', (('H', 256), ('D', 300)), 1), ('dna', (('V', 256), ('D', 300)), 1),
        ('gap', (('Z', 256, 256), ('D', 300)), 1), ('gap', (('Z', 256, 256), ('D', 300)), 2),
        ('gap', (('Z', 256, 256), ('D', 300)), 3), ('gap', (('Z', 256, 256), ('D', 300)), 4),
        ('dna', (('D', 300),), 2), ('dna', (('N', 300),), 3), ('gap', (('Z', 16, 16), ('D', 300)), 1),
        ('gap', (('Z', 16, 16), ('D', 300)), 2), ('gap', (('Z', 16, 16), ('D', 300)), 3),
        ('gap', (('Z', 16, 16), ('D', 300)), 4), ('gap0', (('Z', 150, 150), ('D', 260)), 1),
        ('gap0', (('Z', 150, 150), ('D', 260)), 2),
    ],
    # CORRIDOR: W5
    'CORRIDOR': [
        ('dna', (('D', 1), ('H', 330), ('D', 300)), 1), ('dna', (('D', 1), ('H', 330), ('D', 300)), 2),
        ('dna', (('D', 1), ('V', 330), ('D', 300)), 1), ('dna', (('D', 1), ('V', 330), ('D', 300)), 2),
        ('dna', (('D', 7), ('H', 330), ('D', 300)), 1), ('dna', (('D', 7), ('H', 330), ('D', 300)), 2),
        ('dna', (('D', 7), ('V', 330), ('D', 300)), 1), ('dna', (('D', 7), ('V', 330), ('D', 300)), 2),
        ('dna', (('D', 8), ('H', 330), ('D', 300)), 0), ('dna', (('D', 8), ('H', 330), ('D', 300)), 1),
        ('dna', (('D', 8), ('V', 330), ('D', 300)), 0), ('dna', (('D', 8), ('V', 330), ('D', 300)), 1),
        ('dna', (('D', 16), ('H', 330), ('D', 300)), 0), ('dna', (('D', 16), ('H', 330), ('D', 300)), 2),
        ('dna', (('D', 16), ('V', 330), ('D', 300)), 0), ('dna', (('D', 16), ('V', 330), ('D', 300)), 2),
        ('dna', (('D', 17), ('H', 330), ('D', 300)), 0), ('dna', (('D', 17), ('H', 330), ('D', 300)), 1),
        ('dna', (('D', 17), ('V', 330), ('D', 300)), 0), ('dna', (('D', 17), ('V', 330), ('D', 300)), 1),
        ('dna', (('D', 24), ('H', 330), ('D', 300)), 2), ('dna', (('D', 24), ('V', 330), ('D', 300)), 2),
        ('dna', (('D', 25), ('H', 330), ('D', 300)), 0), ('dna', (('D', 25), ('H', 330), ('D', 300)), 1),
        ('dna', (('D', 25), ('H', 330), ('D', 300)), 2), ('dna', (('D', 25), ('V', 330), ('D', 300)), 0),
        ('dna', (('D', 25), ('V', 330), ('D', 300)), 1), ('dna', (('D', 25), ('V', 330), ('D', 300)), 2),
    ],
    # COUNT: W6; every candidate is kept on purpose (a cover needs 8 of them)
    'COUNT': [
        ('dna', (('D', 511),), 511), ('dna', (('D', 512),), 512), ('dna', (('D', 513),), 513),
        ('dna', (('D', 514),), 514), ('dna', (('D', 200), ('H', 623), ('D', 200)), 1023),
        ('dna', (('D', 200), ('H', 624), ('D', 200)), 1024), ('dna', (('D', 200), ('H', 625), ('D', 200)), 1025),
        ('dna', (('D', 200), ('H', 626), ('D', 200)), 1026), ('dna', (('D', 200), ('H', 1647), ('D', 200)), 2047),
        ('dna', (('D', 200), ('H', 1648), ('D', 200)), 2048), ('dna', (('D', 200), ('H', 1649), ('D', 200)), 2049),
        ('dna', (('D', 200), ('H', 1650), ('D', 200)), 2050), ('dna', (('D', 200), ('H', 1663), ('D', 200)), 2063),
        ('dna', (('D', 200), ('H', 2159), ('D', 200)), 2559),
    ],
    # BANDED: W7
    'BANDED': [
        ('dna', (('D', 65), ('V', 200), ('D', 120)), 0), ('dna', (('D', 64), ('V', 200), ('D', 120)), 2),
        ('dna', (('V', 128), ('N', 250)), 0), ('dna', (('D', 1), ('V', 200), ('D', 120)), 0),
        ('dna', (('V', 128), ('N', 250)), 1), ('dna', (('D', 63), ('V', 200), ('D', 120)), 0),
        ('dna', (('D', 63), ('V', 200), ('D', 120)), 1), ('dna', (('D', 1), ('V', 200), ('D', 120)), 1),
        ('dna', (('D', 1), ('V', 200), ('D', 120)), 2), ('dna', (('D', 2), ('V', 200), ('D', 120)), 0),
        ('dna', (('D', 64), ('V', 200), ('D', 120)), 0), ('dna', (('H', 64), ('N', 250)), 0),
        ('dna', (('H', 64), ('N', 250)), 1),
    ],
    # SLABS: W8
    'SLABS': [
        ('dna', (('D', 200), ('H', 900), ('D', 500)), 0), ('dna', (('D', 513), ('V', 100), ('D', 639)), 0),
        ('dna', (('D', 200), ('H', 900), ('D', 501)), 0), ('dna', (('H', 700), ('N', 701)), 0),
        ('dna', (('H', 700), ('N', 702)), 1), ('dna', (('D', 1024), ('V', 100), ('D', 128)), 0),
        ('dna', (('D', 1025), ('V', 100), ('D', 127)), 0), ('dna', (('H', 1100), ('N', 300)), 0),
        ('dna', (('D', 512), ('V', 100), ('D', 640)), 1), ('dna', (('H', 1100), ('N', 300)), 1),
        ('dna', (('D', 200), ('H', 900), ('D', 502)), 1), ('dna', (('D', 200), ('H', 900), ('D', 503)), 2),
        ('dna', (('H', 700), ('N', 703)), 2),
    ],
}


# which lists a path's tests run, and the condition groups those lists must meet
PATHS = {
    "single": (("RUNS", "ARRIVE", "CORRIDOR", "COUNT"), ("W1", "W2", "W3", "W4", "W5", "W6")),
    "rc": (("RUNS", "ARRIVE", "CORRIDOR", "COUNT", "RC_RUNS"), ("W1", "W2", "W3", "W4", "W5", "W6", "RC")),
    "banded": (("BANDED", "RUNS", "ARRIVE"), ("W7", "W1", "W4")),
    "pipe": (("RUNS", "ARRIVE", "CORRIDOR", "COUNT"), ("W1", "W4", "W5", "W6")),
    "batch": (("RUNS", "ARRIVE", "CORRIDOR", "COUNT"), ("W2", "W3", "W4", "W5", "W6")),
    "slabs": (("SLABS",), ("W8",)),
}


def at_width(base, width, q=0, int8=False):
    """The case of a list entry at a word width (None where its table kind has no such width): the kind's gap open
    costs of the width taken in turn by the entry's index q.  int8: the "gap" table, which leaves the int8 profile
    at o >= 63, gives way to "gap8" at four-byte words."""
    kind, segments, seed = base
    opens = OPENS[kind].get(width)
    if not opens:
        return None
    o = opens[q % len(opens)]
    table = "gap" if kind == "gap0" else kind
    if int8 and table == "gap" and not admissible((cost_table(table, o),)):
        table = "gap8"
    return ((table, o), segments, seed)


def path_cases(path, width, int8=False, names=None):
    """The cases a path's tests run at a word width.  int8: without the cases the int8 query profile refuses;
    path "rc": only cases with m, n >= 256 (the recompute walk's floor); "batch": within the batch route's cells."""
    out = []
    for name in names or PATHS[path][0]:
        for q, base in enumerate(LISTS[name]):
            case = at_width(base, width, q, int8)
            if case is None or (int8 and not admissible((cost_table(*case[0]),))):
                continue
            m, n = shape(case)
            if path == "rc" and min(m, n) < 256:
                continue
            if path == "batch" and m * n > BATCH_CELL_CAP:
                continue
            out.append(case)
    return out


def short(path, width, int8):
    """The named exceptions of a path's list: {class: missing}.  None is left: every class is met by every list."""
    return {}


GOLDEN_CELLS = 400_000


def golden_cases():
    """The cases tests/golden/make_path_golden.py runs the reference on: every list entry under GOLDEN_CELLS cells at
    one-byte words, the first entry of every list whatever its size (one per condition group at the least), the
    first two RUNS and ARRIVE entries at two- and four-byte words, and every ARRIVE entry that takes the "gap8" table
    (the int8 lists at four-byte words)."""
    out = []
    for name, bases in LISTS.items():
        for q, base in enumerate(bases):
            case = at_width(base, 1, q)
            m, n = shape(case)
            if q == 0 or (m + 1) * (n + 1) < GOLDEN_CELLS:
                out.append(case)
    for width in (2, 4):
        for name in ("RUNS", "ARRIVE"):
            out += [at_width(base, width, q) for q, base in enumerate(LISTS[name][:2])]
    out += [c for c in (at_width(base, 4, q, True) for q, base in enumerate(LISTS["ARRIVE"])) if c and c[0][0] == "gap8"]
    return out


# ---------------------------------------------------------------- the search (run by hand; its output is pasted above)
def _flanked(axis, a, g, b, tail="D"):
    return (("D", a), (axis, g), (tail, b))


def candidates():
    """{list name: [(kind, segments, seed)]}: planted templates over a few seeds each; the census decides what a
    candidate reaches (a run slides when its end letters repeat, a Z corner goes either way)."""
    seeds = range(4)
    c = {k: [] for k in ("RUNS", "RC_RUNS", "ARRIVE", "CORRIDOR", "COUNT", "BANDED", "SLABS")}
    # a run of g cells ending on row / column a: (a, a + g) against the seams: 128 | 129 and 512 | 513
    for axis in "HV":
        for a, g in ((128, 384), (128, 385), (129, 383), (129, 384)):
            for s in seeds:
                c["RUNS"].append(("dna", _flanked(axis, a, g, 200, "N" if s & 1 else "D"), s))
    c["RUNS"] += [("dna", (("D", 320),), 0), ("dna", (("N", 321),), 1)]
    c["RC_RUNS"] = [("dna", _flanked("V", 128, 2100, 200), 0), ("dna", _flanked("H", 300, 700, 300), 0)]
    for d in (1, 16, 17, 24, 25, 63, 64, 255, 256, 300):
        for s in seeds:
            c["ARRIVE"] += [("dna", (("H", d), ("D", 300)), s), ("dna", (("V", d), ("D", 300)), s)]
        for s in range(8):
            c["ARRIVE"].append(("gap", (("Z", d, d), ("D", 300)), s))
    c["ARRIVE"] += [("dna", (("D", 300),), 2), ("dna", (("N", 300),), 3)]
    c["ARRIVE"] += [("gap0", (("Z", 150, 150), ("D", 260)), s) for s in (1, 2)]
    for p in (1, 7, 8, 16, 17, 24, 25):
        for axis in "HV":
            for s in seeds:
                c["CORRIDOR"].append(("dna", _flanked(axis, p, 330, 300), s))
    for D in (511, 512, 513, 514):
        c["COUNT"].append(("dna", (("D", D),), D))
    for D in (1023, 1024, 1025, 1026, 2047, 2048, 2049, 2050, 2063, 2559):
        c["COUNT"].append(("dna", _flanked("H", 200, D - 400, 200), D))
    for col in (1, 2, 63, 64, 65):
        for s in seeds:
            c["BANDED"].append(("dna", _flanked("V", col, 200, 120), s))
    for d in (64, 100, 128, 200):
        for s in (0, 1):
            c["BANDED"] += [("dna", (("V", d), ("N", 250)), s), ("dna", (("H", d), ("N", 250)), s)]
    for s in (0, 1, 2):
        c["SLABS"] += [("dna", _flanked("H", 200, 900, 500), s),
                       ("dna", _flanked("V", 512, 100, 640), s), ("dna", _flanked("V", 513, 100, 639), s),
                       ("dna", _flanked("V", 1024, 100, 128), s), ("dna", _flanked("V", 1025, 100, 127), s),
                       ("dna", (("H", 700), ("N", 700)), s), ("dna", (("H", 1100), ("N", 300)), s),
                       ("dna", (("N", 1100), ("H", 300), ("N", 100 + s)), s),
                       ("dna", _flanked("H", 200, 900, 501 + s), s), ("dna", (("H", 700), ("N", 701 + s)), s)]
    return c


SEARCH_GROUPS = {"RUNS": ("W1", "W2", "W3"), "RC_RUNS": ("RC",), "ARRIVE": ("W4",), "CORRIDOR": ("W5",),
                 "COUNT": ("W6",), "BANDED": ("W7",), "SLABS": ("W8",)}


def greedy_cover(cands, groups, width=1, int8=False, start=(), limit=COUNT_CAP):
    """Greedy cover: repeatedly the candidate that removes most of what the groups' conditions still lack, on top
    of the entries of `start`; candidates the width has no table for are left out."""
    cens = {}
    for base in list(start) + [b for b in cands if b not in start]:
        case = at_width(base, width, len(cens), int8)
        if case is not None:
            cens[base] = (case, census(problem(case), case_seed(case)))
    cands = [b for b in cands if b in cens]
    chosen = [b for b in start if b in cens]

    def lack(bases):
        return deficit([cens[b][0] for b in bases], groups, {cens[b][0]: cens[b][1] for b in bases})
    now = lack(chosen)
    while now and len(chosen) < limit:
        best, best_left = None, sum(now.values())
        for b in cands:
            if b in chosen:
                continue
            left = sum(lack(chosen + [b]).values())
            if left < best_left:
                best, best_left = b, left
        if best is None:
            break
        chosen.append(best)
        now = lack(chosen)
    return [b for b in start if b not in cens] + chosen, now


def search():
    """Prints the committed lists: a greedy cover of each list's condition groups over candidates() at one-byte
    words.  ARRIVE is then extended to cover W4 on the int8 lists at four-byte words as well ("gap8", under which
    the Z corners of fewer than 3 letters go by a mismatch) and takes the o = 0 lattice walks on top; COUNT keeps
    every candidate on purpose (a cover needs 8 of the 14 dispatch counts; each one sits at a block or word end)."""
    print("LISTS = {")
    for name, cands in candidates().items():
        chosen, lack = greedy_cover(cands, SEARCH_GROUPS[name])
        if name == "ARRIVE":
            chosen, lack = greedy_cover(cands, SEARCH_GROUPS[name], 4, True, chosen)
            chosen += [b for b in cands if b[0] == "gap0"]
        if name == "COUNT":
            chosen = list(cands)
        print(f"    # {name}: {len(chosen)} cases for {', '.join(SEARCH_GROUPS[name])}; lack {lack}")
        print(f"    {name!r}: [")
        for b in chosen:
            print(f"        {b!r},")
        print("    ],")
    print("}")


def geometry_row(items):
    """One row of the geometry table over [(problem, seed)]: longest interior run per level (cells, seams), longest
    run anywhere, corner moves, largest off-diagonal reach, longest stretch within 16 of an edge, largest D."""
    best = {1: (0, 0), 2: (0, 0)}
    anywhere, corners, reach, near, dmax = 0, 0, 0, 0, 0
    for prob, seed in items:
        cen = census(prob, seed)
        for L, length, first, last, seams, d in cen.runs:
            anywhere = max(anywhere, length)
            if d >= 64 and min(last) >= 64:
                best[L] = max(best[L], (length, seams))
        corners += len(cen.corners)
        reach = max(reach, cen.reach)
        near = max(near, cen.corridors[("row", 16)][0], cen.corridors[("col", 16)][0])
        dmax = max(dmax, cen.D)
    return best[1], best[2], anywhere, corners, reach, near, dmax


def existing_census(max_cells=8_000_000):
    """Prints the geometry table of the walk inputs the suite had before this module and of this module's lists
    (DESIGN.md 2 holds the output; nothing asserts on it)."""
    from oracle import transform
    from tests import tie_classes as tc
    from tests.conftest import splitmix_seq

    def gprob(case):
        s1, s2 = gc.sequences(case)
        return gc.table(case[0], case[1]), s1, s2, case[4]

    def dna(m, n, sa, sb, seed, o=5):
        kw = dict(match_score=2, mismatch_score=-3, gap_open_score=-o, gap_extension_score=-1)
        s1, s2 = splitmix_seq(m, sa, "dna"), splitmix_seq(n, sb, "dna")
        a1, a2, _, cmat, _, goc = transform.settings(dict(kw, seq_1=s1, seq_2=s2))
        return (cmat, a1, a2, goc), seed

    def shapes(m, n):
        rng = random.Random(m * 1000 + n)
        s1 = "".join(rng.choice("ACGT") for _ in range(m))
        s2 = "".join(rng.choice("ACGT") for _ in range(n))
        return (cost_table("dna", 5), s1, s2, 5), m + n

    a = splitmix_seq(2000, 61, "dna")
    planted = [(splitmix_seq(1000, 62, "dna") + a + splitmix_seq(1000, 63, "dna"), 61, False),
               (splitmix_seq(700, 64, "dna") + a + splitmix_seq(900, 65, "dna"), 62, True)]
    lists = {
        "test_gpu_parity shapes": [shapes(m, n) for m, n in ((2, 2), (3, 70), (63, 64), (64, 65), (65, 63), (100, 449),
                                                             (449, 100), (448, 448), (130, 1000), (1000, 130),
                                                             (777, 1555), (2049, 1023))],
        "general_costs.ROW_WALK": [(gprob(c), c[2] ^ c[3]) for c in gc.ROW_WALK],
        "general_costs.RC": [(gprob(c), c[2] + c[4]) for c, _, _ in gc.RC],
        "general_costs.BANDED": [(gprob(c), c[3] ^ b) for c, b in gc.BANDED],
        "tie_classes lists": [(tc.scaled_problem(c, k), tc.case_seed(c)) for c, k in tc.width_cases(1)],
        "test_gpu_rc DNA inputs": [dna(m, n, 11, 12, m + n) for m, n in ((256, 256), (300, 500), (1000, 1300),
                                                                         (777, 2049), (2049, 3000))],
        "test_gpu_rc long gap runs": [((cost_table("dna", 5), other, a, 5) if flip else
                                       (cost_table("dna", 5), a, other, 5), seed) for other, seed, flip in planted],
    }
    for path in ("single", "rc", "banded", "slabs"):
        lists[f"path_geometry {path}"] = [(problem(c), case_seed(c)) for c in path_cases(path, 1)]
    print("| case list | cases | longest interior level-1 run (cells, seams) | level-2 | longest run anywhere | "
          "corner moves | tile reach | longest stretch within 16 of an edge | largest D |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, items in lists.items():
        items = [(p, s) for p, s in items if (len(p[1]) + 1) * (len(p[2]) + 1) <= max_cells]
        r1, r2, anywhere, corners, reach, near, dmax = geometry_row(items)
        print(f"| {name} | {len(items)} | {r1[0]}, {r1[1]} | {r2[0]}, {r2[1]} | {anywhere} | {corners} | {reach} | "
              f"{near} | {dmax} |")


if __name__ == "__main__":
    search()
