"""The device route of align_pairs' tie-break tables without a GPU: the block-level pieces batch_rng_kernel is made of
(globalign_amd/csrc/ga_batch_rng.h) in a CPU model that runs them lane by lane as the kernel does, against the host's
tables -- a stand-alone self-test, plain and under AddressSanitizer + UndefinedBehaviorSanitizer -- and the ``tables``
argument of GlobalAligner.align_pairs: checked before the sequences and before any engine exists, handed to the engine
as a keyword of its own for "device", and not at all for "host"."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "globalign_amd", "csrc")
LIB = os.path.join(ROOT, "globalign_amd", "_lib")


@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-s", "-C", CSRC, "batch_rng_selftest", "batch_rng_asan"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return True


@pytest.mark.parametrize("binary", ["ga_batch_rng_selftest_asan", "ga_batch_rng_selftest"])
def test_block_model_selftest(built, binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(LIB, binary)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_exports():
    from globalign_amd import _native
    lib = _native.load_library()
    for name in ("ga_batch_align_ex", "ga_batch_align_info", "ga_debug_pair_tables"):
        assert name in _native.EXPORTS and hasattr(lib, name)


@pytest.fixture
def no_engine(monkeypatch):
    from globalign_amd import _native

    def refuse(*args, **kwargs):
        raise AssertionError("an engine was asked for before validation finished")

    monkeypatch.setattr(_native, "default_engine", refuse)
    monkeypatch.setattr(_native, "Engine", refuse)
    import globalign_amd
    return globalign_amd


@pytest.mark.parametrize("tables", ["gpu", "Device", "", None, 2, b"device"])
def test_bad_tables_value_comes_before_the_sequences(no_engine, tables):
    """ValueError for anything but "host" / "device", although the lists are of unequal length, a sequence holds a gap
    and a seed is negative: the argument is checked first."""
    with pytest.raises(ValueError) as e:
        no_engine.GlobalAligner().align_pairs(["ACGT", "A-"], ["ACGT"], seeds=-1, tables=tables)
    assert "tables" in str(e.value)
    with pytest.raises(ValueError) as e:
        no_engine.GlobalAligner().align_pairs(["AC-T"], ["ACGT"], tables=tables)
    assert "tables" in str(e.value)


@pytest.mark.parametrize("tables", ["host", "device"])
def test_good_tables_value_leaves_validation_as_it_was(no_engine, tables):
    with pytest.raises(RuntimeError):
        no_engine.GlobalAligner().align_pairs(["ACGT", "AC-T"], ["ACGT", "ACGT"], tables=tables)
    res = no_engine.GlobalAligner().align_pairs([], [], tables=tables)
    assert res.costs.shape == (0,)


def _recorder(seen):
    class Recorder:
        # (the engine's call as the existing fakes take it: `tables` here are the cost tables)
        def batch_align(self, codes, seq_off, pair_a, pair_b, tables, seeds, chars, pair_max_cost=None, **more):
            seen.update(more=dict(more), cost_tables=tables, seeds=seeds)
            P = len(pair_a)
            bufs = tuple(np.frombuffer(t, dtype=np.uint8) for t in (b"AC-TxxAA", b"|| |yy* ", b"ACGTzzC-"))
            return (np.arange(P, dtype=np.int64), np.zeros(P, dtype=np.int32), np.array([4, 2], dtype=np.int64),
                    np.array([0, 6, 8], dtype=np.int64), bufs)

    return Recorder


def test_device_reaches_the_engine_as_its_own_keyword(monkeypatch):
    import globalign_amd
    from globalign_amd import _native
    seen = {}
    monkeypatch.setattr(_native, "default_engine", lambda device=0: _recorder(seen)())
    res = globalign_amd.GlobalAligner().align_pairs(["acgt", "AA"], ["ACGT", "A"], seeds=3, tables="device")
    assert seen["more"] == {"rng_tables": "device"}
    assert isinstance(seen["cost_tables"], _native.CostTables) and seen["seeds"].tolist() == [3, 4]
    assert res.seq_1_aligned == ["AC-T", "AA"]


@pytest.mark.parametrize("kw", [{}, {"tables": "host"}])
def test_host_reaches_the_engine_with_no_new_keyword(monkeypatch, kw):
    import globalign_amd
    from globalign_amd import _native
    seen = {}
    monkeypatch.setattr(_native, "default_engine", lambda device=0: _recorder(seen)())
    globalign_amd.GlobalAligner().align_pairs(["acgt", "AA"], ["ACGT", "A"], **kw)
    assert seen["more"] == {}


def test_engine_refuses_an_unknown_route():
    """Engine.batch_align and Engine.debug_pair_tables check their route before they touch the context."""
    from globalign_amd import _native
    eng = object.__new__(_native.Engine)
    z = np.zeros(1, dtype=np.uint8)
    with pytest.raises(ValueError):
        eng.batch_align(z, [0, 1], [0], [0], None, [0], z, rng_tables="gpu")
    with pytest.raises(ValueError):
        eng.debug_pair_tables([0], [1], rng_tables=None)
