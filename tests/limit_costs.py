"""Cost tables at the limits the host checks admit, and the cases the GPU parity tests run under them
(tests/test_gpu_limits.py; tests/test_limit_costs_cpu.py checks on the CPU that the cases can fail, that they reach
the magnitudes they are meant to reach, and pins the oracle against the reference at these magnitudes).

The host proves that a problem is safe for the int32 kernels and picks their data widths (ga_check.h: range_fits,
profile_bytes, tb_word_bytes; load_problem; the batch planner).  The tables of tests/general_costs.py stay far inside
every one of those limits; the families here sit on them.  The guard is restated below from ga_check.h, not called.

Families (keys in dict order, '-' last, every key one character).  A case is (family, variant, m, n, gap open cost):

  P8    K = 5, sub' = sub - gap_v - gap_h holds +127 and -127, the -127 entries are the four matches; int8 profile.
        P8+a: one mismatch entry at sub' = +128; P8+b: one match entry at -128 -- both int16 profiles.
  P16   the same at +-32767 (int16).  P16+a / P16+b: one entry at +32768 / -32768: the single call refuses, the batch
        kernels read 4-byte table entries.
  Kn    K = n keys (n - 1 letters and '-'): sub from 0..9 per entry, a gap cost per letter that differs from its
        neighbours' and from the letter's 32 codes below, in both directions.  variant = the gap costs' scale: 1 an
        int8 profile, 5 int16, 600 past int16.  Letters are printable ASCII up to K = 91, other characters beyond
        (score only).  Every code occurs in both sequences where they are long enough, the last letter code always;
        the highest codes sit on both sides of position 64 (a stripe edge, row 64).
  V16   K = 5, match 0 / mismatch 5 / gaps 2-3 (ties everywhere) times the largest factor the int16 profile and the
        guard admit at the case's shape.  V32: the same past int16, up to the guard (batches, 4-byte entries).
  Vphi  gap costs G + small distinct offsets, sub = gap_v + gap_h + (-127..+127): an int8 profile while GV, GH, big
        and the cost's un-shift are as large as the guard admits.  V-: the same with G < 0 (falling prefix sums, rising
        shifted values, a negative cost).  The factor is |G|.
  VB+   a general_costs G table under caller-supplied row 0 / column 0 triples drawn from [B - 400, B] (VB-: from
        [-B, -B + 400]), corner triple 0, B the largest value the guard admits at the shape.  variant = table seed.
"""
import functools
import random

from tests import general_costs as gc

LETTERS = gc.LETTERS
M64 = gc.M64
INT32_MAX = 2 ** 31 - 1
O_MAX = 32766  # the largest gap open cost a traceback word holds: its 15-bit fields take values up to o + 1


# ---------------------------------------------------------------- ga_check.h, restated
def range_bound(bmax, m, n, maxabs, gap_open):
    return bmax + (m + n + 2) * (3 * maxabs + gap_open)


def range_fits(bound):
    return 4 * bound < INT32_MAX


def costs_maxabs(cmat):
    return max(abs(v) for row in cmat.values() for v in row.values())


def max_cost(cmat):
    return max(max(row.values()) for row in cmat.values())


def shifted_sub(cmat):
    """sub' = sub - gap_v - gap_h over every key pair, '-' included (what profile_bytes looks at)."""
    return {x: {y: cmat[x][y] - cmat[x]["-"] - cmat["-"][y] for y in cmat} for x in cmat}


def profile_bytes(cmat):
    big = max(abs(v) for row in shifted_sub(cmat).values() for v in row.values())
    return 1 if big <= 127 else 2 if big <= 32767 else 0


def tb_word_bytes(o):
    return 1 if o + 1 < 8 else 2 if o + 1 < 128 else 4 if o + 1 < 32768 else 0


def guard_fits(cmat, m, n, o, boundary_max=0):
    """check_problem's int32 range guard (boundary_max: the largest |value| of caller-supplied boundary triples)."""
    big = (max_cost(cmat) + 1) * max(m, n)
    return range_fits(range_bound(max(abs(big), boundary_max), m, n, costs_maxabs(cmat), o))


def single_accepts(cmat, m, n, o):
    """What check_problem accepts: the guard, an int8 / int16 profile and a traceback word for o."""
    return guard_fits(cmat, m, n, o) and profile_bytes(cmat) != 0 and tb_word_bytes(o) != 0


def batch_accepts(cmat, m, n, o):
    """What the batch planner accepts of a pair: the guard and the word; the profile may need 4-byte entries."""
    return guard_fits(cmat, m, n, o) and tb_word_bytes(o) != 0


# ---------------------------------------------------------------- K = 5 tables
def _from_shifted(d, gh, gv):
    """The costing dict whose sub' is d (4 x 4) under the gap costs gh, gv."""
    return gc._dict([[d[i][j] + gv[i] + gh[j] for j in range(4)] for i in range(4)], gh, gv)


def p_table(family, seed=1):
    """P8 / P8+a / P8+b / P16 / P16+a / P16+b."""
    wide = family.startswith("P16")
    cap, unit = (32767, 100) if wide else (127, 1)
    rng = random.Random(11_000_000 + seed + (16 if wide else 8))
    gv = [20 * unit, 25 * unit, 31 * unit, 40 * unit]
    gh = [23 * unit, 28 * unit, 35 * unit, 43 * unit]
    d = [[-cap if i == j else rng.randint(-(cap // 2), cap - 1) for j in range(4)] for i in range(4)]
    d[0][1] = cap
    if family.endswith("+a"):
        d[2][3] = cap + 1
    elif family.endswith("+b"):
        d[1][1] = -(cap + 1)
    else:
        assert family in ("P8", "P16"), family
    cmat = _from_shifted(d, gh, gv)
    sp = shifted_sub(cmat)
    vals = [sp[x][y] for x in LETTERS[:-1] for y in LETTERS[:-1]]
    assert len(set(gh)) == 4 and len(set(gv)) == 4 and gh != gv
    assert cap in vals and all(sp[x][x] <= -cap for x in LETTERS[:-1])
    assert profile_bytes(cmat) == {"P8": 1, "P8+a": 2, "P8+b": 2, "P16": 2, "P16+a": 0, "P16+b": 0}[family]
    return cmat


def v16_table(f):
    """match 0 / mismatch 5 / gaps 2-3, times f: sub' is -5f on the diagonal and within +-f off it."""
    gv, gh = [2 * f, 3 * f, 2 * f, 3 * f], [3 * f, 2 * f, 3 * f, 2 * f]
    return gc._dict([[0 if i == j else 5 * f for j in range(4)] for i in range(4)], gh, gv)


_PHI_D = [[-127, 127, 12, 6], [12, -127, 5, 12], [6, 12, -127, -3], [127, 0, 12, -127]]


def vphi_table(G):
    """gap costs G + small distinct offsets, sub' = _PHI_D (int8, +-127 both present, ties between a mismatch at 12
    and two gaps opened at 6) whatever G is."""
    gv, gh = [G + 1, G + 4, G + 6, G + 9], [G + 2, G + 3, G + 7, G + 8]
    cmat = _from_shifted(_PHI_D, gh, gv)
    assert profile_bytes(cmat) == 1
    return cmat


def _v_table(family, f):
    return {"V16": v16_table, "V32": v16_table, "Vphi": vphi_table, "V-": lambda g: vphi_table(-g)}[family](f)


@functools.lru_cache(maxsize=None)
def v_factor(family, m, n, o):
    """The largest factor of a V family that its acceptance admits at this shape (V16: the single call's, which the
    int16 profile caps; V32: the batch planner's; Vphi, V-: the single call's, capped by the guard)."""
    ok = batch_accepts if family == "V32" else single_accepts
    lo, hi = 1, 2 ** 29
    assert ok(_v_table(family, lo), m, n, o) and not ok(_v_table(family, hi), m, n, o)
    while hi - lo > 1:  # (every acceptance is monotone in the factor)
        mid = (lo + hi) // 2
        if ok(_v_table(family, mid), m, n, o):
            lo = mid
        else:
            hi = mid
    return lo


def v_table(family, m, n, o, excess=0):
    """The family's table at its largest factor for the shape; excess = 1: at the first factor that is refused."""
    return _v_table(family, v_factor(family, m, n, o) + excess)


# ---------------------------------------------------------------- large alphabets
def k_keys(K):
    """K - 1 letters and '-': printable ASCII (without '-') while it lasts, then characters from U+0100 on."""
    ascii_letters = [chr(c) for c in range(33, 127) if chr(c) != "-"]
    letters = ascii_letters[:K - 1] if K - 1 <= len(ascii_letters) else [chr(0x100 + c) for c in range(K - 1)]
    return letters + ["-"]


@functools.lru_cache(maxsize=None)
def k_table(K, scale=1):
    keys = k_keys(K)
    rng = random.Random(12_000_000 + K)
    gv = [1 + scale * ((7 * x + 3) % 61) for x in range(K - 1)]
    gh = [1 + scale * ((11 * y + 5) % 59) for y in range(K - 1)]
    cmat = {x: {y: rng.randint(0, 9) for y in keys[:-1]} for x in keys[:-1]}
    for i, x in enumerate(keys[:-1]):
        cmat[x]["-"] = gv[i]
    cmat["-"] = {y: gh[j] for j, y in enumerate(keys[:-1])}
    cmat["-"]["-"] = 0
    for g in (gv, gh):  # a neighbouring row or column, or the code's low five bits, is another gap cost
        assert all(g[x] != g[x - 1] for x in range(1, K - 1)) and all(g[x] != g[x & 31] for x in range(32, K - 1))
    assert gv[:4] != gh[:4] and profile_bytes(cmat) == {1: 1, 5: 2, 600: 0}[scale]
    return cmat


def k_seq(length, K, seed):
    """`length` letter codes of a K-key alphabet as a string: SplitMix64 draws, a permutation of every code from
    position 0, the eight highest codes over positions 60..67, then any code still missing put where a repeated one
    stood (past position 68)."""
    keys = k_keys(K)
    nl = K - 1
    state, codes = seed & M64, []
    for _ in range(length):
        state = (state + 0x9E3779B97F4A7C15) & M64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        codes.append(((z ^ (z >> 31)) >> 32) * nl >> 32)
    perm = list(range(nl))
    random.Random(seed).shuffle(perm)
    for q in range(min(length, nl)):
        codes[q] = perm[q]
    for q in range(60, min(68, length)):
        codes[q] = nl - 1 - (q - 60) % min(8, nl)
    codes[length - 1 if length < 61 else 60] = nl - 1  # the last letter code, whatever the length
    count = [0] * nl
    for c in codes:
        count[c] += 1
    q = 68
    for c in range(nl):
        if count[c]:
            continue
        while q < length and count[codes[q]] < 2:
            q += 1
        if q >= length:
            break
        count[codes[q]] -= 1
        codes[q] = c
        count[c] = 1
        q += 1
    return "".join(keys[c] for c in codes)


def all_codes_occur(s, K):
    return set(s) == set(k_keys(K)[:-1])


# ---------------------------------------------------------------- cases -> problems
def family_K(family):
    return int(family[1:]) if family[0] == "K" else 5


def table(case):
    family, variant, m, n, o = case
    if family[0] == "P":
        return p_table(family, variant)
    if family[0] == "K":
        return k_table(family_K(family), variant)
    if family in ("VB+", "VB-"):
        return gc.general_table(variant)
    return v_table(family, m, n, o)


def _base_seed(case):
    family, variant, m, n, o = case
    h = 0
    for ch in family:
        h = (h * 131 + ord(ch)) & M64
    return ((h * 1_000_003 + variant) * 1_000_003 + m * 7919 + n * 104_729 + o) & M64


def sequences(case):
    family, _, m, n, _ = case
    base = _base_seed(case)
    if family[0] == "K":
        K = family_K(family)
        return k_seq(m, K, base), k_seq(n, K, base + 1)
    return gc.splitmix_seq(m, base), gc.splitmix_seq(n, base + 1)


def problem(case):
    """(costing dict, seq_1, seq_2, gap open cost) of a case."""
    s1, s2 = sequences(case)
    return table(case), s1, s2, case[4]


def vb_bound(case):
    """B of a VB case: the largest boundary magnitude the guard admits at its shape."""
    family, variant, m, n, o = case
    cmat = gc.general_table(variant)
    B = (INT32_MAX - 1) // 4 - (m + n + 2) * (3 * costs_maxabs(cmat) + o)
    assert guard_fits(cmat, m, n, o, B) and not guard_fits(cmat, m, n, o, B + 1)
    return B


def vb_boundary(case):
    """(row0, col0) of a VB case as flat lists of 3 (n + 1) and 3 (m + 1) values."""
    family, variant, m, n, o = case
    B = vb_bound(case)
    rng = random.Random(_base_seed(case))
    lo, hi = (B - 400, B) if family == "VB+" else (-B, -B + 400)
    row0 = [rng.randint(lo, hi) for _ in range(3 * (n + 1))]
    col0 = [rng.randint(lo, hi) for _ in range(3 * (m + 1))]
    row0[:3] = col0[:3] = [0, 0, 0]
    row0[3], col0[3] = hi if family == "VB+" else lo, lo if family == "VB+" else hi  # both ends of the range occur
    return row0, col0


def is_v(case):
    return case[0][0] == "V"


# ---------------------------------------------------------------- corruptions a wrong kernel would amount to
def _map_shifted(cmat, fn):
    """A copy of cmat whose letter x letter sub' entries went through fn."""
    out = {x: dict(row) for x, row in cmat.items()}
    for x in cmat:
        for y in cmat:
            if x != "-" and y != "-":
                out[x][y] = fn(cmat[x][y] - cmat[x]["-"] - cmat["-"][y]) + cmat[x]["-"] + cmat["-"][y]
    return out


def _wrap(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


TABLE_CORRUPTIONS = {
    "int8-zero-extended": lambda v: v + 256 if v < 0 else v,
    "int16-low-int8": lambda v: _wrap(v, 8),
    "int16-zero-extended": lambda v: v + 65536 if v < 0 else v,
    "int32-low-int16": lambda v: _wrap(v, 16),
    "int32-low-uint16": lambda v: v & 0xFFFF,
}


def corrupt_table(cmat, kind):
    return _map_shifted(cmat, TABLE_CORRUPTIONS[kind])


def corrupt_codes(s, K, kind):
    """"low5": code x read as x & 31; "last": the last letter's code x read as x - 1."""
    keys = k_keys(K) if K != 5 else LETTERS
    code = {k: i for i, k in enumerate(keys)}
    if kind == "low5":
        return "".join(keys[code[ch] & 31] for ch in s)
    assert kind == "last"
    return s.replace(keys[K - 2], keys[K - 3])


def table_corruptions(cmat):
    """The table corruptions that apply to a table, by its profile width: [("table", kind)]."""
    qb = profile_bytes(cmat)
    out = [("table", k) for k in {1: ["int8-zero-extended"], 2: ["int16-low-int8", "int16-zero-extended"],
                                  0: ["int32-low-int16", "int32-low-uint16"]}[qb]
           if corrupt_table(cmat, k) != cmat]  # (-128 / -32768 is its own low byte / half: P8+b and P16+b take the unsigned read only)
    assert out
    return out


def corruptions(case):
    """The corruptions that apply to a case: [("table", kind) or ("codes", kind)], by what the kernels read for it --
    the profile width, and for a Kn family the code width (x & 31 needs a letter code of 32 or more: K >= 34)."""
    family = case[0]
    out = table_corruptions(table(case))
    if family[0] == "K":
        out.append(("codes", "last"))
        if family_K(family) >= 34:
            out.append(("codes", "low5"))
    return out


def corrupted_cost(case, what, kind):
    cmat, s1, s2, o = problem(case)
    if what == "table":
        return gc.oracle_cost(corrupt_table(cmat, kind), s1, s2, o)
    K = family_K(case[0])
    return gc.oracle_cost(cmat, corrupt_codes(s1, K, kind), corrupt_codes(s2, K, kind), o)


def eligible(case):
    """As general_costs.eligible; the VB cases (a cost under caller-supplied boundaries) are checked cell by cell on
    the GPU and take no part."""
    return gc.eligible(case) and case[0] not in ("VB+", "VB-")


# ---------------------------------------------------------------- the GPU cases, by path
def _cases(fams, shapes, opens):
    return [f + (m, n, o) for f in fams for (m, n) in shapes for o in opens]


P8, P8A, P8B, P16, P16A, P16B = ("P8", 1), ("P8+a", 1), ("P8+b", 1), ("P16", 1), ("P16+a", 1), ("P16+b", 1)
V16, V32, VPHI, VNEG, VBP, VBN = ("V16", 0), ("V32", 0), ("Vphi", 0), ("V-", 0), ("VB+", 1), ("VB-", 1)


def K_(n, scale=1):
    return ("K%d" % n, scale)


# every cell, row scan.  V16 reaches 2^25 only from about 1000 letters a side on (its factor is capped by the int16
# profile, not by the guard), so its shape is the batches' 1100 x 600
FULL_CELLS = (_cases([P8, P16], [(70, 130), (130, 321)], [6]) + [K_(64) + (130, 321, 6), V16 + (1100, 600, O_MAX)])
FULL_CELLS_CUSTOM = [VBP + (130, 321, 6), VBN + (130, 321, 6), VBP + (70, 130, O_MAX)]
# row scan + walk at one-, two- and four-byte words (the K families: m above 1100, so that a ring of 512 or 256
# profile rows wraps several times; V16 where it reaches 2^25)
WALK_OPENS = (6, 126, O_MAX)
ROW_WALK = (_cases([P8A, P16], [(65, 130), (300, 449)], WALK_OPENS) + _cases([P8B], [(65, 130)], WALK_OPENS)
            + _cases([V16], [(1100, 600)], WALK_OPENS) + _cases([VPHI], [(130, 1000)], WALK_OPENS)
            + _cases([K_(33), K_(64), K_(90), K_(90, 5)], [(1150, 130)], WALK_OPENS)
            + _cases([K_(33), K_(64)], [(65, 130)], [O_MAX]))
ROW_RING_SHAPE = (1150, 300)  # the largest loadable alphabet: a ring of 128 rows wraps eight times
LANE_TDS = (1, 2, 4, 8)


def lane_shapes(td):
    return [(300, 64 * td * 5 + 3), (17, 513)]


def lane_handover_shape(td):
    return (300, 64 * td * 9 + 77)  # ten stripes: three workgroups of four waves


def lane_score_cases(td):
    """Two families per (TD, NWC) over the path's shapes, and a three-workgroup case of each lane family at TD 2."""
    fams = {1: [P8, VPHI], 2: [VNEG, K_(32)], 4: [VPHI, K_(32)], 8: [P8, VNEG]}[td]
    out = _cases(fams, lane_shapes(td), [6])
    if td == 2:
        out += _cases([P8, VPHI, VNEG, K_(32)], [lane_handover_shape(2)], [6])
    return out


LANE_DECLINED = _cases([P8A, P8B, K_(33), K_(64)], [(300, 64 * 5 + 3)], [6])  # int16 profile / K > 32: the row scan
LANE_CUSTOM = [VBP + (300, 64 * 2 * 5 + 3, 6), VBN + (300, 64 * 2 * 9 + 77, 6)]
LANE_HANDOVER = VPHI + lane_handover_shape(2) + (6,)


def lane_walk_cases(td):
    return _cases([P8, VPHI, K_(32)], [(200, 64 * td * 4 + 77)], [5])


DIAG = _cases([P8], [(300, 2049)], [6]) + [V16 + (1100, 2049, 6)]
# recompute walk: (case, columns per lane or None, GA_RC_EVERY or None)
RC = [(P8 + (777, 2049, 7), 1, None), (VPHI + (777, 2049, 7), 2, None), (VNEG + (2049, 700, 5), 4, None),
      (K_(32) + (777, 2049, 5), 8, None), (VPHI + (2049, 700, 130), None, None), (P8 + (2049, 700, 7), None, 128),
      (VNEG + (777, 2049, 5), None, 128), (K_(32) + (2049, 700, 5), None, None),
      # (four-byte words: a recompute worker's block fits LDS at up to 2 columns per lane, plan_rc_fill narrows wider)
      (VPHI + (777, 2049, O_MAX), 2, None)]
RC_DECLINED = [P8A + (777, 2049, 5), P8B + (777, 2049, 5), K_(33) + (777, 2049, 5), K_(64) + (777, 2049, 5)]
BANDED = [(P8 + (777, 2049, 5), 64), (V16 + (4096, 1024, 5), 16), (VPHI + (777, 2049, 20), 64),
          (VPHI + (4096, 1024, O_MAX), 16)]
PIPELINE = _cases([VPHI, P8], [(900, 1000)], [5])
SLABS = VPHI + (1500, 3 * 512 + 77, 5)

# batches: the general tables' corner shapes, cut per family to what the guard allows
BATCH_COST_SHAPES = list(gc._CORNERS) + [(1100, 600), (70, 5000)]
BATCH_ALIGN_SHAPES = list(gc.BATCH_ALIGN_SHAPES)
V32_SHAPES = [(65, 70), (70, 65), (3, 130), (64, 64), (2, 70)]
# a V family's batch runs under one table, so its factor is the largest pair's: 1100 x 600, where V16 reaches 2^25
V_BATCH_SHAPES = list(gc._CORNERS) + [(1100, 600)]
# the large alphabets: every code fits both sides of the first shape at K = 255; m above 1100 in the last
K_BATCH_SHAPES = [(300, 310), (65, 129), (257, 64), (3, 65), (127, 513), (1150, 300)]


def batch_cases(fam, shapes, o):
    """fam over `shapes`, those the batch planner's guard refuses under the family's table left out."""
    out = []
    for m, n in shapes:
        case = fam + (m, n, o)
        if not is_v(case) and not batch_accepts(table(case), m, n, o):
            continue
        out.append(case)
    return out


def v_batch_cases(fam, shapes, o):
    """A V family in a batch: one table for every pair, at the largest factor the batch's largest pair admits (the
    pairs' own maxima differ; the planner checks each pair under the one table)."""
    f = min(v_factor(fam[0], m, n, o) for m, n in shapes)
    return _v_table(fam[0], f), [fam + (m, n, o) for m, n in shapes], f


def all_single_cases():
    """Every single-call case the GPU tests run under the reference's own boundary, once each."""
    out = list(FULL_CELLS) + list(ROW_WALK) + list(LANE_DECLINED) + [LANE_HANDOVER, SLABS] + list(DIAG) + list(PIPELINE)
    for td in LANE_TDS:
        out += lane_score_cases(td)
    for td in (1, 2, 4):
        out += lane_walk_cases(td)
    out += [c for c, _, _ in RC] + list(RC_DECLINED) + [c for c, _ in BANDED]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


def all_custom_cases():
    return list(FULL_CELLS_CUSTOM) + list(LANE_CUSTOM)
