"""A plain ``bench.py --gpus 1`` run on the GPU: the lean result line and ``--dump-outputs``.

One run of the smallest workload (C1, 1k x 1k DNA, full traceback; cost 2471, BASELINE.md golden results)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    e = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "cells/s" and line["higher_is_better"] is True and line["dtype"] == "int32"
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e6 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["config"]["cost"] == 2471
    # what takes runs or references of its own is behind --full
    for key in ("cpu_baseline", "c4", "pipelined_repeated_pair", "roofline"):
        assert key not in line
    assert "traceback_pin" not in line["config"]
    # the dump: what the last timed step returned
    import bench
    s1, s2 = bench.workload_pair(bench.WORKLOADS["c1"])
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sorted(got) == ["cost", "middle_part", "random_state_after", "seq_1_aligned", "seq_2_aligned", "status"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["cost"].tolist() == [2471.0] and got["status"].tolist() == [0.0]
    a, mid, b = (bytes(got[k].astype(np.uint8)).decode() for k in ("seq_1_aligned", "middle_part", "seq_2_aligned"))
    assert len(a) == len(mid) == len(b) and a.replace("-", "") == s1 and b.replace("-", "") == s2
    assert got["random_state_after"].shape in ((624,), (625,))
