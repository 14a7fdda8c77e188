"""The decoder set's C ABI and hvite's switches for it, without a GPU: the symbols are exported and declared in htk_amd/capi.py, `-w`
without a network name is taken by option parsing, `-w` (no name) together with `-a` is refused as the reference refuses
loadNetworks && loadLabels (HVite.c:453)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "golden", "decode", "bigram")
SYMS = ("htkamd_decoder_set_create", "htkamd_decoder_set_destroy", "htkamd_decoder_set_run", "htkamd_decoder_set_last_tied")


@pytest.fixture(scope="module")
def hvite(native):
    from htk_amd import build as nbuild
    nbuild.build_tools()
    return os.path.join(ROOT, "tools", "bin", "hvite")


def test_decoder_set_symbols_are_exported_and_declared(native):
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "htk_amd.h")).read()
    for s in SYMS:
        assert hasattr(L, s), s
        assert s + "(" in header, s
    assert "DoAlignment" in header and "HVite.c:830" in header
    assert issubclass(native.DecoderSet, object) and hasattr(native.DecoderSet, "run")
    # bad arguments are refused before a device is needed
    assert L.htkamd_decoder_set_create(None, None, 0, 1.0, None) == -1
    assert b"decoder_set_create" in L.htkamd_last_error()
    assert L.htkamd_decoder_set_run(None, None, None, None, None, 0, 1, None, None) == -1
    assert L.htkamd_decoder_set_last_tied(None) == 0


def _run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_hvite_takes_w_without_a_network_name(native, hvite):
    tail = [os.path.join(SRC, "dict"), os.path.join(SRC, "hmmlist"), "nosuch.mfc"]
    for w in (["-w", "-L", "lat", "-X", "lat"], ["-L", "lat", "-w", "", "-X", "lat"], ["-L", "lat", "-X", "lat", "-w", "-t", "250.0"]):
        r = _run([hvite, "-H", os.path.join(SRC, "MMF")] + w + tail)
        assert r.returncode != 0
        assert "value expected" not in r.stderr and "either -w net or -a" not in r.stderr and "unknown switch" not in r.stderr, (w, r.stderr)
        if native.lib().htkamd_device_count() <= 0:
            assert "no HIP device" in r.stderr, (w, r.stderr)         # parsing and the checks behind it went through
    r = _run([hvite, "-w", "-n", "4", "-L", "lat", "-X", "lat"] + tail)
    assert r.returncode != 0 and "lattice per file" in r.stderr        # N-best over a set: out of scope, said so


def test_hvite_refuses_w_without_a_name_together_with_a(hvite):
    tail = [os.path.join(SRC, "dict"), os.path.join(SRC, "hmmlist"), "nosuch.mfc"]
    for w in (["-a", "-w", "-L", "lat"], ["-w", "", "-a"], ["-w", "-a"]):
        r = _run([hvite] + w + tail)
        assert r.returncode != 0 and "not together with -a" in r.stderr, (w, r.stderr)
