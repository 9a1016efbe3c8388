"""The repeated-alignment pipeline without a GPU: its pure part (globalign_amd/csrc/ga_pipe.h -- the knob parse, the
plan of a call, the thread that feeds the tie-break table ahead of the walks) in a stand-alone self-test, plain, under
AddressSanitizer + UndefinedBehaviorSanitizer, and under ThreadSanitizer for the feeder's protocol."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "globalign_amd", "csrc")
LIB = os.path.join(ROOT, "globalign_amd", "_lib")


@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-s", "-C", CSRC, "pipe_selftest", "pipe_asan", "pipe_tsan"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return True


@pytest.mark.parametrize("binary", ["ga_pipe_selftest_asan", "ga_pipe_selftest_tsan", "ga_pipe_selftest"])
def test_host_selftest(built, binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(LIB, binary)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "ThreadSanitizer" not in r.stderr
