"""The lean steady-state loop of the recompute fill (ga_lane.hip, iterations [it_lo, it_hi)) at the places it can
go wrong, on the default 2-column stripes and on the other widths: its bounds (the smallest problem, a partial last
stripe of 1 and of 127 columns), the staircase checkpoint's `done < m` edge around a multiple of 64, rings that wrap
many times, many stripes linked inside and across workgroups, and the paths around it (the masked ramp, the
compiler's steps, caller-supplied boundaries).  Every case is the recompute path (GA_RC=1) against the oracle: cost,
the three strings and the random state (test_gpu_rc._align)."""
import random

import numpy as np
import pytest

from tests.conftest import splitmix_seq, set_knob
from tests.test_gpu_rc import DNA, _align

pytestmark = pytest.mark.gpu


def _dna(monkeypatch, m, n, env=None):
    return _align(monkeypatch, splitmix_seq(m, 3 * m + 1, "dna"), splitmix_seq(n, 5 * n + 2, "dna"), DNA,
                  seed=m + n, env=env)


@pytest.mark.parametrize("m,n", [(256, 256), (319, 300), (320, 300), (321, 300), (2047, 385), (2048, 511),
                                 (12000, 600), (300, 6000)])
def test_loop_bounds_and_exits_vs_oracle(monkeypatch, m, n):
    """(256, 256) the smallest accepted; m = 319 / 320 / 321 the staircase's `done < m` edge; n = 385 and 511 a last
    stripe of 1 and of 127 columns at 2 columns per lane; 12000 rows wrap every ring many times; 6000 columns are 47
    stripes, so links inside and across workgroups and a start lag on each."""
    assert _dna(monkeypatch, m, n)[1] == 2


@pytest.mark.parametrize("td", [1, 2, 4])
@pytest.mark.parametrize("m,n", [(2047, 385), (300, 6000)])
def test_loop_widths_vs_oracle(monkeypatch, m, n, td):
    assert _dna(monkeypatch, m, n, {"GA_LANE_COLS_PER_LANE": td})[1] == td


@pytest.mark.parametrize("env", [{"GA_LANE_LEAN0": 0}, {"GA_LANE_ASM": 0}])
def test_old_paths_vs_oracle(monkeypatch, env):
    """The masked ramp before the lean loop, and the compiler's steps instead of it."""
    assert _dna(monkeypatch, 2500, 2600, env)[1] == 2


def test_caller_boundaries_turn_lean0_off_vs_oracle(monkeypatch):
    """Boundaries passed to ga_problem_set (here the reference's own, so the oracle's alignment still holds): the host
    cannot assume a uniform row 0, and the fill takes the masked ramp."""
    from globalign_amd import _native
    from globalign_amd.scoring import validate_and_transform_args
    from oracle import core, transform
    m, n = 2500, 2600
    s1, s2 = splitmix_seq(m, 47, "dna"), splitmix_seq(n, 48, "dna")
    a1, a2, smat, cmat, gos, goc = transform.settings(dict(DNA, seq_1=s1, seq_2=s2))
    random.seed(9)
    mt = np.array(random.getstate()[1], dtype=np.uint32)
    ref = core.align(a1, a2, cmat, goc, mt)
    tab = core.Tables(cmat)
    row0, col0 = core.boundary(tab, tab.codes(a1), tab.codes(a2), goc, (tab.max_cost + 1) * max(m, n))
    _, _, _, cmat2, _, goc2, _ = validate_and_transform_args(None, None, s1[:64], s2[:64], **DNA)
    tables = _native.CostTables(cmat2, goc2)
    set_knob(monkeypatch, "GA_RC", "1")
    eng = _native.Engine(0)
    try:
        eng.load(tables.codes(a1), tables.codes(a2), tables, row0=row0, col0=col0)
        cost, strings, status, mt_after = eng.align(mt, a1, a2)
        kind = eng.fill_kind()
    finally:
        eng.close()
    assert kind[0] == "rc" and kind[1] == 2, kind
    assert status == 0 and int(cost) == ref["cost"]
    assert tuple(strings) == tuple(ref["strings"])
    assert np.asarray(mt_after, dtype=np.uint32).tolist() == np.asarray(ref["mt_out"], dtype=np.uint32).tolist()


def test_protein_blosum62_vs_oracle(monkeypatch):
    kw = dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)
    kind = _align(monkeypatch, splitmix_seq(1200, 3, "protein"), splitmix_seq(1400, 4, "protein"), kw, seed=3,
                  protein=True)
    assert kind[1] == 4, kind


def test_checkpoint_spacing_128_vs_oracle(monkeypatch):
    """A staircase checkpoint every fourth iteration of the loop, not every second."""
    assert _dna(monkeypatch, 3000, 3500, {"GA_RC_EVERY": 128})[1] == 2
