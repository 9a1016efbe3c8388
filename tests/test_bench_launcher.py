"""bench.py's multi-rank launcher on CPU: ``--gpus N`` without a launcher starts N ranks itself.

The ranks run the real slab orchestration over gloo with the oracle-backed CPU engine
(tests/bench_cpu_engine.py); rank 0 prints ONE JSON line with n_gpus == N and the C1 cost
(2471, BASELINE.md golden results)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env):
    e = dict(os.environ, PYTHONPATH=ROOT, **env)
    e.pop("WORLD_SIZE", None)
    e.pop("RANK", None)
    e.pop("LOCAL_RANK", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, capture_output=True,
                          text=True, timeout=600)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_bench_spawns_ranks_gloo(n):
    """World sizes up to the driver's 8-GPU node: 8 ranks over gloo (C1's 1000 columns cut into slabs as narrow as
    one column: the orchestration's edge cases)."""
    r = _run(["--gpus", str(n), "--workload", "c1", "--steps", "2", "--warmup", "1"], GA_DIST_BACKEND="gloo",
             GA_BENCH_ENGINE="tests.bench_cpu_engine:make_engine")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == n and line["steps"] == 2 and line["warmup"] == 1
    assert line["config"]["cost"] == 2471 and line["config"]["backend"] == "gloo"
    assert line["value"] > 0 and line["slab_fill_ms_max"] > 0
    assert sum(line["slab_columns"]) == 1000
    # the edge preflight: every boundary's transport in the line (CPU engines relay bands)
    pre = line["config"]["edge_links"]
    assert len(pre["boundaries"]) == n - 1 and not pre["ipc_agreed"]
    assert all(b["transport"].startswith("bands") for b in pre["boundaries"])


def test_bench_refuses_missing_gpus():
    """No silent single-rank run: with the RCCL backend and fewer GPUs than asked, exit non-zero."""
    r = _run(["--gpus", "2", "--workload", "c1"], GA_DIST_BACKEND="nccl", HIP_VISIBLE_DEVICES="")
    assert r.returncode != 0
    assert "needs 2 visible GPUs" in r.stderr


def test_bench_refuses_world_mismatch():
    e = dict(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "c1"],
                       env=dict(os.environ, PYTHONPATH=ROOT, **e), capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "launcher started 1 ranks" in r.stderr


def test_dump_outputs_writes_what_the_step_returned(tmp_path, monkeypatch):
    """--dump-outputs: one float64 .npy per output of the last timed step, every value exact; an output past the size
    limit is cut to the same seeded sample of its elements in every run."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    mt = np.arange(625, dtype=np.uint32) * np.uint32(6700417)  # words up to 2^32: exact in float64, not in float32
    r = {"cost": 2471, "aln": ("AC-GT", "|| .|", "ACTCT"), "status": 0, "mt_after": mt}
    bench.dump_outputs(str(tmp_path / "a"), r)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["cost", "middle_part", "random_state_after", "seq_1_aligned", "seq_2_aligned", "status"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["cost"].tolist() == [2471.0] and got["status"].tolist() == [0.0]
    assert bytes(got["seq_1_aligned"].astype(np.uint8)).decode() == "AC-GT"
    assert bytes(got["middle_part"].astype(np.uint8)).decode() == "|| .|"
    assert bytes(got["seq_2_aligned"].astype(np.uint8)).decode() == "ACTCT"
    assert np.array_equal(got["random_state_after"].astype(np.uint32), mt)
    # a score-only step returns its cost alone
    bench.dump_outputs(str(tmp_path / "s"), {"cost": 7})
    assert os.listdir(tmp_path / "s") == ["cost.npy"] and np.load(tmp_path / "s" / "cost.npy").tolist() == [7.0]
    # past the limit: a sample of budget elements per array, in order, the same in every run
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 6 * 8 * 100)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), dict(r, aln=("A" * 500 + "C" * 500,) * 3))
    b, c = (np.load(tmp_path / d / "seq_1_aligned.npy") for d in ("b", "c"))
    assert b.shape == (84,) and np.array_equal(b, c) and np.all(np.diff(b) >= 0) and set(b.tolist()) == {65.0, 67.0}
    assert np.array_equal(np.load(tmp_path / "b" / "random_state_after.npy"), np.load(tmp_path / "c" / "random_state_after.npy"))
    total = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert total <= 6 * 8 * 100  # the files, headers included, within the limit


def test_roofline_profiles_must_match_the_variant_that_ran():
    """bench.roofline divides the committed profile's SQ_INSTS_VALU per launch by the fill's measured time: only when
    the profile (and its VALU mix) are of the kernel variant that ran (columns per lane), else achieved stays null."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench._variant_td("void ga::fill_lane_kernel<4, 2, 0, 16, false, false, true, true>(ga::FillArgs)") == 2
    assert bench._variant_td("_ZN2ga16fill_lane_kernelILi4ELi8ELi0ELi16ELb0ELb0ELb0ELb0EEEvNS_8FillArgsE") == 8
    assert bench._variant_td("fill_kernel") is None
    c3 = bench.WORKLOADS["c3"]
    ok = bench.roofline("c3", c3, 7.6, fill_kind=("rc", 4, 391, 4, 98))
    assert "profile_mismatch" not in ok and 0 < ok["frac"] < 1
    bad = bench.roofline("c3", c3, 6.8, fill_kind=("rc", 2, 782, 4, 196))
    assert bad["achieved"] is None and bad["frac"] is None and "profile_mismatch" in bad
