"""The recompute fill's default stripe width (ga_plan.h plan_rc_fill): 2 columns per lane for
alphabets of <= 8 codes whose 128-column stripes all run at once (<= 4 per CU), 4 otherwise; GA_RC_NARROW=0 restores
4 for an A/B run and GA_LANE_COLS_PER_LANE overrides both.  The width is fill_kind()[1]; every case is also held
to the oracle (cost, the three strings, the random state) by test_gpu_rc._align."""
import pytest

from tests.conftest import splitmix_seq
from tests.test_gpu_rc import DNA, _align

pytestmark = pytest.mark.gpu


def _dna(monkeypatch, env):
    return _align(monkeypatch, splitmix_seq(2500, 41, "dna"), splitmix_seq(2600, 42, "dna"), DNA, seed=7, env=env)


def test_default_is_two_columns_for_dna(monkeypatch):
    assert _dna(monkeypatch, None)[1] == 2


def test_narrow_0_restores_four_columns(monkeypatch):
    assert _dna(monkeypatch, {"GA_RC_NARROW": 0})[1] == 4


def test_protein_keeps_four_columns(monkeypatch):
    kw = dict(scoring_mat_name="BLOSUM62", gap_open_score=-10)
    kind = _align(monkeypatch, splitmix_seq(1200, 3, "protein"), splitmix_seq(1400, 4, "protein"), kw, seed=3,
                  protein=True)
    assert kind[1] == 4, kind


def test_more_stripes_than_simds_keeps_four_columns(monkeypatch):
    """131,300 columns are 1026 stripes of 128: more than the 4 per CU (1024 on 256 CUs) that run at once."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 131_300
    assert (n + 127) // 128 > 4 * ncu, ncu
    kind = _align(monkeypatch, splitmix_seq(256, 43, "dna"), splitmix_seq(n, 44, "dna"), DNA, seed=8)
    assert kind[1] == 4, kind


def test_cols_per_lane_overrides_narrow(monkeypatch):
    assert _dna(monkeypatch, {"GA_LANE_COLS_PER_LANE": 4, "GA_RC_NARROW": 1})[1] == 4
