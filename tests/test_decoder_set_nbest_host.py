"""N-best token sets and lattices over a decoder set, without a GPU: the C ABI (htkamd_decoder_set_run_lattice[_align]) is exported,
declared and refuses bad arguments before a device is needed; hvite takes -n together with -a and with a lattice per file; and the
fixtures of tests/golden/decode/set_nbest -- the reference's HVite in DoAlignment with several tokens -- are what the oracle's token-set
decoder gives, utterance by utterance over that utterance's own network, through the product's lattice writer and N-best code."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from set_nbest_util import INDEX, SRC, TAGS, bigram_mmf, check_files, load_case, with_prons

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("htkamd_decoder_set_run_lattice", "htkamd_decoder_set_run_lattice_align")


@pytest.fixture(scope="module")
def hvite(native):
    from htk_amd import build as nbuild
    nbuild.build_tools()
    return os.path.join(ROOT, "tools", "bin", "hvite")


def test_set_lattice_symbols_are_exported_and_declared(native):
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "htk_amd.h")).read()
    for s in SYMS:
        assert hasattr(L, s), s
        assert s + "(" in header, s
    assert hasattr(native.DecoderSet, "run_lattice")


def test_set_lattice_bad_arguments_are_refused_before_a_device_is_needed(native):
    """NULLs and nToks outside 2..8 need no set (a set cannot be made without a device; netOf out of range, which needs one, is in
    tests/test_gpu_decoder_set_nbest.py)."""
    L = native.lib()
    cfg = native.DecodeConfig(1.0e10, 1.0e10, 1.0, 0.0, 1.0, 0, 0)
    nn = np.zeros(1, np.int32); na = np.zeros(1, np.int32)
    out = native.LatticeOut(nn.ctypes.data_as(C.c_void_p), na.ctypes.data_as(C.c_void_p), *([None] * 11))
    fo = np.zeros(2, np.int32).ctypes.data_as(C.c_void_p)
    for nToks in (3, 1, 9):
        assert L.htkamd_decoder_set_run_lattice(None, C.byref(cfg), nToks, 10.0, None, fo, fo, 1, 100, 100, C.byref(out), None) == -1
        msg = L.htkamd_last_error()
        assert b"decoder_set_run_lattice" in msg and (nToks == 3 or (b"nToks = %d" % nToks) in msg), msg
        assert L.htkamd_decoder_set_run_lattice_align(None, C.byref(cfg), nToks, 10.0, 1, None, fo, fo, 1, 100, 100, 100, C.byref(out), None, None) == -1
        msg = L.htkamd_last_error()
        assert b"decoder_set_run_lattice" in msg and (nToks == 3 or (b"nToks = %d" % nToks) in msg), msg
    assert L.htkamd_decoder_set_run_lattice(None, None, 3, 10.0, None, None, None, 0, 100, 100, None, None) == -1
    assert b"decoder_set_run_lattice" in L.htkamd_last_error()


def _run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_hvite_takes_n_with_a_and_with_a_lattice_per_file(native, hvite):
    head = [hvite, "-H", os.path.join(SRC, "MMF")]
    tail = [os.path.join(SRC, "dict"), os.path.join(SRC, "hmmlist"), "nosuch.mfc"]
    for sw in (["-a", "-n", "3", "-z", "lat"], ["-w", "-n", "3", "3", "-L", "d", "-X", "lat"], ["-a", "-n", "3", "2", "-m"], ["-a", "-f", "-n", "2", "-z", "lat"],
               ["-w", "-L", "d", "-X", "lat", "-n", "4", "-z", "lt2", "-l", "out"]):
        r = _run(head + sw + tail)
        assert r.returncode != 0
        for refusal in ("value expected", "either -w net or -a", "unknown switch", "not supported", "lattice per file", "tokens per state"):
            assert refusal not in r.stderr, (sw, r.stderr)
        if native.lib().htkamd_device_count() <= 0:
            assert "no HIP device" in r.stderr, (sw, r.stderr)          # parsing and the checks behind it went through
    # neither lattices nor alternatives asked for: the one refusal that stays, and it says what to add
    r = _run(head + ["-w", "-n", "4", "-L", "lat", "-X", "lat"] + tail)
    assert r.returncode != 0 and "lattice per file" in r.stderr and "-z" in r.stderr and "N > 1" in r.stderr, r.stderr
    r = _run(head + ["-w", "-n", "9", "3", "-L", "lat", "-X", "lat"] + tail)
    assert r.returncode != 0 and "2..8 tokens per state" in r.stderr, r.stderr


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_per_utterance_network_and_host_lattice_code_equal_hvite(native, oracle, tag, tmp_path):
    """Needs no device and none of the set's new entry points: it pins the fixtures and the host code (the lattice writer's form for a lattice
    without an lmname among it) that the device path is then compared through."""
    mmf = bigram_mmf(native)
    c, nets, feats, p, align = load_case(native, mmf, tag)
    om = oracle.Model(mmf.packed())
    arcs = failed = 0
    for u, (X, net) in enumerate(zip(feats, nets)):
        lat = oracle.decode_nbest(om, X, net.arrays(), c["nToks"], align=align, **p)
        if "u%d" % u not in c["nbest"]:                              # (-u took every token before the final node: HVite wrote nothing)
            assert lat is None, (tag, u)
            failed += 1
            continue
        assert lat is not None, (tag, u)
        lat = with_prons(lat, net)
        lat.update(lmScale=p["lmScale"], wordPen=p["wordPen"], prScale=p["prScale"], alignModels=bool(align & 1))
        check_files(native, lat, net, mmf, tag, u, tmp_path)
        arcs += len(lat["arcStart"])
    assert arcs > 20 and failed == c["n"] - len(c["nbest"])
    assert failed == (1 if tag == "rescore_u" else 0)
