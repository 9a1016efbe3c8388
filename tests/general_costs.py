"""Letter-dependent, asymmetric cost tables and the cases the GPU parity tests run under them
(tests/test_gpu_general_costs.py; tests/test_oracle.py checks on the CPU that the cases can fail).

Every fill works in a shifted domain, V' = V - GV(i) - GH(j) and sub' = sub - gap_v[a] - gap_h[b],
which differs from plain arithmetic only when the gap costs depend on the letter and gap_h, gap_v and the two
triangles of sub differ from each other.  Three deterministic table families over A C G T and '-' (in this key
order, '-' last), each from a seed:

  G  general, int8 profile: sub[x][y] drawn independently from 0..9 (asymmetric, non-zero diagonal), gap_h four
     distinct values from 1..9, gap_v four other distinct values from 1..9.
  W  wide and signed, int16 profile: sub from -50..200, gap_h and gap_v four distinct values each from -20..150.
  S  reachable through the public API: a symmetric score matrix with each row's maximum on the diagonal and a
     different gap score per letter (as tests/golden/make_golden.py's mtx mode draws it), written to a .mtx file.

A case is (family, table seed, m, n, gap open cost); its sequences are SplitMix64 draws over ACGT.
"""
import random

LETTERS = ["A", "C", "G", "T", "-"]
M64 = (1 << 64) - 1


def splitmix_seq(length, seed):
    """tests/conftest.py's generator over ACGT (restated: tests/golden/make_general_golden.py imports this module
    without pytest)."""
    state = seed & M64
    out = []
    for _ in range(length):
        state = (state + 0x9E3779B97F4A7C15) & M64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z = z ^ (z >> 31)
        out.append("ACGT"[z >> 62])
    return "".join(out)


def gap_h(cmat):
    return [cmat["-"][y] for y in LETTERS[:-1]]


def gap_v(cmat):
    return [cmat[x]["-"] for x in LETTERS[:-1]]


def max_abs_shifted_sub(cmat):
    """max |sub'| = |sub[x][y] - gap_v[x] - gap_h[y]| over every key pair, '-' included: what ga_check.h's
    profile_bytes looks at."""
    keys = list(cmat.keys())
    return max(abs(cmat[x][y] - cmat[x]["-"] - cmat["-"][y]) for x in keys for y in keys)


def profile_bytes(cmat):
    """ga_check.h profile_bytes: bytes of a query-profile entry, 1 or 2 by the largest |sub'|, 0 past int16."""
    big = max_abs_shifted_sub(cmat)
    return 1 if big <= 127 else 2 if big <= 32767 else 0


def _dict(sub, gh, gv):
    L = LETTERS[:-1]
    cmat = {x: {y: sub[i][j] for j, y in enumerate(L)} for i, x in enumerate(L)}
    for i, x in enumerate(L):
        cmat[x]["-"] = gv[i]
    cmat["-"] = {y: gh[j] for j, y in enumerate(L)}
    cmat["-"]["-"] = 0
    return cmat


def _check_general(cmat, family):
    gh, gv = gap_h(cmat), gap_v(cmat)
    L = LETTERS[:-1]
    assert list(cmat.keys()) == LETTERS and all(list(row.keys()) == LETTERS for row in cmat.values())
    assert len(set(gh)) == 4 and len(set(gv)) == 4 and gh != gv, (family, gh, gv)
    assert any(cmat[x][y] != cmat[y][x] for x in L for y in L), family
    if family == "G":
        assert max_abs_shifted_sub(cmat) <= 127 and profile_bytes(cmat) == 1
    else:
        assert max_abs_shifted_sub(cmat) > 127 and profile_bytes(cmat) == 2
    return cmat


def general_table(seed):
    rng = random.Random(7_000_000 + seed)
    sub = [[rng.randint(0, 9) for _ in range(4)] for _ in range(4)]
    gaps = rng.sample(range(1, 10), 8)
    return _check_general(_dict(sub, gaps[:4], gaps[4:]), "G")


def wide_table(seed):
    rng = random.Random(8_000_000 + seed)
    sub = [[rng.randint(-50, 200) for _ in range(4)] for _ in range(4)]
    return _check_general(_dict(sub, rng.sample(range(-20, 151), 4), rng.sample(range(-20, 151), 4)), "W")


def api_score_rows(seed):
    """(letters, rows of scores) of family S: symmetric, off-diagonal -6..1, diagonal 2..7 (make_golden.py's mtx
    mode), redrawn until the four gap scores differ."""
    rng = random.Random(9_000_000 + seed)
    K = len(LETTERS)
    while True:
        S = [[0] * K for _ in range(K)]
        for x in range(K):
            for y in range(x, K):
                S[x][y] = S[y][x] = rng.randint(-6, 1)
        for x in range(K):
            S[x][x] = rng.randint(2, 7)
        if len(set(S[K - 1][:K - 1])) == 4:
            return list(LETTERS), S


def write_mtx(path, letters, rows):
    with open(path, "w") as fh:
        fh.write("  ".join(letters) + "\n")
        for x, row in zip(letters, rows):
            fh.write(x + " " + " ".join(str(v) for v in row) + "\n")
    return str(path)


def api_tables(seed):
    """Family S on the oracle's side -> (scoring dict, costing dict), through the oracle's restated transform."""
    from oracle import transform
    letters, rows = api_score_rows(seed)
    smat = transform.read_mtx_rows(letters, rows)
    cmat = transform.scores_to_costs(smat, transform.max_val(smat))
    assert len(set(gap_h(cmat))) == 4 and len(set(gap_v(cmat))) == 4 and gap_h(cmat) != gap_v(cmat)
    assert profile_bytes(cmat) == 1
    return smat, cmat


def table(family, seed):
    """The costing dict of a case's family and table seed."""
    return {"G": general_table, "W": wide_table, "S": lambda s: api_tables(s)[1]}[family](seed)


def sequences(case):
    family, seed, m, n, o = case
    base = ((ord(family) * 1_000_003 + seed) * 1_000_003 + m * 7919 + n * 104_729 + o) & M64
    return splitmix_seq(m, base), splitmix_seq(n, base + 1)


# ---------------------------------------------------------------- corruptions a wrong kernel would amount to
def corrupt(cmat, kind):
    """A copy of cmat with (a) "swap": gap_h and gap_v swapped; (b) "transpose": sub transposed; (c) "rotate": the
    gap costs rotated by one letter (A gets C's, ..., T gets A's)."""
    L = LETTERS[:-1]
    out = {x: dict(row) for x, row in cmat.items()}
    if kind == "swap":
        for x in L:
            out[x]["-"], out["-"][x] = cmat["-"][x], cmat[x]["-"]
    elif kind == "transpose":
        for x in L:
            for y in L:
                out[x][y] = cmat[y][x]
    elif kind == "rotate":
        for k, x in enumerate(L):
            nxt = L[(k + 1) % 4]
            out[x]["-"], out["-"][x] = cmat[nxt]["-"], cmat["-"][nxt]
    else:
        raise ValueError(kind)
    return out


CORRUPTIONS = ("swap", "transpose", "rotate")


def oracle_cost(cmat, s1, s2, o):
    """min of the last cell of the oracle's boundary + score fill under cmat."""
    from oracle import core
    tab = core.Tables(cmat)
    a, b = tab.codes(s1), tab.codes(s2)
    big = (tab.max_cost + 1) * max(len(a), len(b))
    row0, col0 = core.boundary(tab, a, b, o, big)
    return int(min(core.fill_score(tab, a, b, o, row0, col0)))


def eligible(case):
    """The discrimination condition applies to cases with unequal sides of at least 17 letters."""
    _, _, m, n, _ = case
    return m != n and min(m, n) >= 17


# ---------------------------------------------------------------- the GPU cases, by path
# (W seed 1 draws a negative gap_v entry, W seed 7 a negative gap_h entry: GV / GH are not monotone there)
G1, G2, G3, W1, W2, S1 = ("G", 1), ("G", 2), ("G", 3), ("W", 1), ("W", 7), ("S", 1)


def _cases(fams, shapes, opens):
    return [f + (m, n, o) for f in fams for (m, n) in shapes for o in opens]


# every cell, row scan (Engine.fill(full=True) against core.fill_full)
FULL_CELLS = _cases([G1, W1], [(70, 130), (130, 321)], [6])
# row scan + walk at the default geometry
ROW_WALK = _cases([G1, W1], [(65, 130), (300, 449), (130, 1000)], [3, 20, 300])
# lane fill, score only: shapes by columns per lane TD
LANE_TDS = (1, 2, 4, 8)


def lane_score_cases(td):
    return _cases([G2, W2], [(17, 513), (300, 64 * td * 5 + 3), (5, 130)], [6])


# lane fill with traceback words + walk (G at TD 1, 2, 4; W at TD 2)
def lane_walk_cases(td):
    fams = [G2, W2] if td == 2 else [G2]
    return _cases(fams, [(200, 64 * td * 4 + 77), (1000, 1300)], [5])


LANE_HANDOVER = G2 + (300, 64 * 2 * 5 + 77, 6)
# anti-diagonal fill (the lean ramp's own case: lean_ramp_case() below)
DIAG = _cases([G3], [(300, 2049), (31, 64)], [6])
# recompute walk: (case, columns per lane or None, GA_RC_EVERY or None)
RC = [(G1 + (256, 256, 5), 1, None), (G1 + (777, 2049, 7), 2, None), (G1 + (2049, 700, 5), 4, None),
      (G1 + (777, 2049, 5), 8, None), (G1 + (2049, 700, 130), None, None), (G1 + (2049, 700, 7), None, 128),
      (W1 + (777, 2049, 5), None, None)]
# banded traceback: (case, GA_TB_BAND_ROWS)
BANDED = [(G3 + (300, 500, 5), 16), (G3 + (300, 500, 5), 64), (G3 + (777, 2049, 20), 96), (G3 + (777, 2049, 5), 16),
          (G3 + (4096, 1024, 5), 16), (W2 + (777, 2049, 20), 64)]
# pipeline (Engine.align_many, count 3)
PIPELINE = _cases([G1], [(900, 1000), (2000, 64)], [5])
# slabs in one process
SLABS = G2 + (1500, 3 * 512 + 77, 5)
# public API (family S)
API = _cases([S1], [(449, 1000), (130, 321)], [6])

# batches: the corner shapes of tests/test_gpu_batch.py / test_gpu_batch_align.py, then further mixes of their
# EDGE_LENGTHS up to 24 pairs, then the shapes named for the edge column in LDS / in HBM
_CORNERS = [(64, 64), (65, 129), (63, 257), (256, 255), (257, 64), (3, 65), (128, 128), (129, 127), (127, 513),
            (300, 300), (2, 300), (300, 3), (513, 513)]
_MIXES = [(255, 65), (64, 513), (513, 63), (129, 300), (257, 127), (3, 256), (128, 2), (65, 64)]
BATCH_COST_SHAPES = [(1, 1), (1, 513), (513, 1)] + _CORNERS + _MIXES + [(70, 5000), (1100, 600)]
BATCH_ALIGN_SHAPES = [(2, 2), (2, 513), (513, 2)] + _CORNERS + _MIXES + [(1100, 600)]
BATCH_OPEN = {"G": 5, "W": 20, "S": 6}


def batch_cases(shapes, fam):
    return [fam + (m, n, BATCH_OPEN[fam[0]]) for m, n in shapes]


BATCH_API_SHAPES = [(2, 2), (2, 513), (513, 2)] + _CORNERS + _MIXES[:4]


def all_gpu_cases():
    """Every (family, seed, m, n, gap open) the GPU tests run, once each."""
    out = list(FULL_CELLS) + list(ROW_WALK) + [LANE_HANDOVER, SLABS] + list(DIAG) + list(PIPELINE) + list(API)
    for td in LANE_TDS:
        out += lane_score_cases(td)
    for td in (1, 2, 4):
        out += lane_walk_cases(td)
    out += [c for c, _, _ in RC] + [c for c, _ in BANDED]
    for fam in (G3, W2):
        out += batch_cases(BATCH_COST_SHAPES, fam) + batch_cases(BATCH_ALIGN_SHAPES, fam)
    out += batch_cases(BATCH_API_SHAPES, S1)
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


def lean_ramp_case():
    """A lane-mode score case on which the lean ramp's two predicates differ: gap_h = {A, C, G: 150, T: -20}, so
    GH(j) rises over seq_2's 35 letters from ACG and falls over its 35 T; with gap open 4600 and max_cost 200,
    big = 201 * 70 = 14070 and 2o + GH(35) = 14450 > big >= 2o + GH(70) = 13750.  sub stays within an int8 profile
    (the lane fill's), with maximum 200.  -> (cmat, seq_1, seq_2, o)"""
    gh, gv = [150, 150, 150, -20], [50, 40, 45, 30]
    sub = [[200, 140, 120, 60], [130, 150, 110, 70], [125, 135, 160, 50], [115, 145, 105, 90]]
    cmat = _dict(sub, gh, gv)
    o = 4600
    s1 = splitmix_seq(5, 77)
    s2 = "".join("ACG"["ACGT".index(ch) % 3] for ch in splitmix_seq(35, 78)) + "T" * 35
    big = (max(max(r.values()) for r in cmat.values()) + 1) * 70
    GH = [0]
    for ch in s2:
        GH.append(GH[-1] + cmat["-"][ch])
    assert profile_bytes(cmat) == 1 and big == 14070
    assert 2 * o + GH[35] == 14450 > big >= 2 * o + GH[70] == 13750 and max(GH) == GH[35]
    return cmat, s1, s2, o
