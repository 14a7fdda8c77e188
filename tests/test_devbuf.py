"""csrc/devbuf.h and csrc/hipcheck.h on their own: tests/devbuf_selftest.hip, a stand-alone program that htk_amd/build.py compiles into
tools/bin, exercises the typed buffer, the scratch list, the kernel timer and the accumulating check.  With a device it round-trips
1 / 63 / 64 / 65 ints and 1 / 1000 doubles bit for bit, checks the empty rule, the grow-only reserve, the reusable timer and the scratch
list's distinct pointers; without one every reserve / upload / get returns an error code, leaves p == nullptr and cap == 0, names its
owner in the last error, and everything is destroyed cleanly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "bin", "devbuf_selftest")


def _run():
    assert os.path.exists(EXE), "tools/bin/devbuf_selftest is not built (python -m htk_amd.build)"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_without_a_device_every_call_fails_cleanly(native):
    if native.lib().htkamd_device_count() > 0:
        pytest.skip("a GPU is visible")
    assert "devbuf selftest ok (no device)" in _run()


@pytest.mark.gpu
def test_buffer_scratch_and_timer_on_the_device():
    assert "devbuf selftest ok (device)" in _run()
