"""The FFT front ends beyond MFCC on the device: PLP, FBANK and MELSPEC coded from waveforms (htkamd_frontend_*, capi.FrontEnd, the
drivers' waveform sources) against the reference's HCopy (tests/golden/wave/frontend_*.conf -> test_<KIND>.<case>.htk, written by
tests/golden/make_frontend_golden.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "wave")
BIN = os.path.join(ROOT, "tools", "bin")
HCOPY = os.path.join(ROOT, "oracle", "_ref", "HCopy")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_frontend_golden as g  # noqa: E402

# configuration variable -> frontend_config keyword (value parser)
_VARS = {"SOURCERATE": ("sampPeriod", float), "WINDOWSIZE": ("winDur", float), "TARGETRATE": ("frPeriod", float),
         "NUMCHANS": ("numChans", int), "NUMCEPS": ("numCeps", int), "CEPLIFTER": ("cepLifter", int), "PREEMCOEF": ("preEmph", float),
         "USEHAMMING": ("useHam", "bool"), "USEPOWER": ("usePower", "bool"), "ZMEANSOURCE": ("zMeanSource", "bool"),
         "ENORMALISE": ("eNormalise", "bool"), "RAWENERGY": ("rawEnergy", "bool"), "LPCORDER": ("lpcOrder", int),
         "COMPRESSFACT": ("compressFact", float), "CEPSCALE": ("cepScale", float)}


def case_config(native, case):
    """frontend_config of golden case `case` from its committed configuration text (HParm's defaults for what it does not set)."""
    kw, kind = {"usePower": False, "eNormalise": True, "numChans": 20}, None
    for line in open(os.path.join(GOLD, "frontend_%s.conf" % case)):
        k, v = (x.strip() for x in line.split("="))
        if k == "TARGETKIND":
            kind = v
        elif k in _VARS:
            name, typ = _VARS[k]
            kw[name] = (v[0] in "Tt") if typ == "bool" else typ(v)
    return native.frontend_config(kind, **kw), kind


def golden(native, case):
    ref, period, kind = native.parm_read(os.path.join(GOLD, g.out_name(case)))
    assert period == 100000
    return ref


def bit_share(got, ref):
    return float((got == ref).mean())


def assert_matches(kind, got, ref):
    """FBANK / MELSPEC: the MFCC rule (test_wave.py); PLP: the same tolerance, at least 99 % of the values bit-equal (the device's double
    pow / log against the host's)."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.allclose(got, ref, rtol=1e-4, atol=1e-3), np.abs(got - ref).max()
    share = bit_share(got, ref)
    if kind.startswith("PLP"):
        assert share >= 0.99, share
    else:
        assert share > 0.999, share


# ---------------------------------------------------------------------------------------------------------------- host only
@pytest.mark.parametrize("case,cols", [("a", 39), ("d", 123), ("f", 26)])
def test_num_cols_match_the_golden_headers(native, case, cols):
    cfg, _ = case_config(native, case)
    assert native.frontend_num_cols(cfg) == cols
    assert golden(native, case).shape[1] == cols


@pytest.mark.parametrize("kind,kw,why", [
    ("LPC", {}, "LPC is a time-domain LPC kind"),
    ("LPREFC", {}, "LPREFC is a time-domain LPC kind"),
    ("LPCEPSTRA_E", {}, "LPCEPSTRA is a time-domain LPC kind"),
    ("FBANK_0", {}, "_0 on FBANK"),
    ("MELSPEC_0_D", {}, "_0 on MELSPEC"),
    ("PLP_0", {"lpcOrder": 1}, "LPCORDER 1"),
    ("PLP_0", {"lpcOrder": 1001, "numCeps": 12}, "LPCORDER 1001"),
    ("PLP_0", {"numCeps": 13}, "NUMCEPS 13"),
    ("PLP_0", {"numCeps": 1}, "NUMCEPS 1"),
    ("PLP_0", {"compressFact": 1.0}, "COMPRESSFACT"),
    ("PLP_0", {"compressFact": 0.0}, "COMPRESSFACT"),
    ("FBANK", {"numChans": 1}, "NUMCHANS"),
    ("MELSPEC", {"numChans": 1001}, "NUMCHANS"),
    ("PLP_E", {"winDur": 100.0}, "geometry"),
])
def test_refused_configurations(native, kind, kw, why):
    cfg = native.frontend_config(kind, **kw)
    with pytest.raises(native.HtkAmdError, match=re.escape(why)):
        native.frontend_num_cols(cfg)
    # create refuses with the same reason before it looks for a device
    h = C.c_void_p()
    assert native.lib().htkamd_frontend_create(C.byref(cfg), C.byref(h)) == -1
    assert why in native.lib().htkamd_last_error().decode()


def test_unknown_base_kind_is_refused(native):
    cfg = native.frontend_config("MFCC")
    cfg.baseKind = 9                                              # USER
    with pytest.raises(native.HtkAmdError, match="not an FFT front end"):
        native.frontend_num_cols(cfg)


def test_mfcc_through_the_frontend_counts_as_mfcc(native):
    for kind, ch in (("MFCC_0_D_A", 26), ("MFCC_E_D_A_Z", 40)):
        assert native.frontend_num_cols(native.frontend_config(kind, numChans=ch)) == native.lib().htkamd_mfcc_num_cols(
            C.byref(native.mfcc_config(kind, numChans=ch)))


@pytest.mark.parametrize("tool", ["herest", "hvite"])
def test_drivers_refuse_lpc_kinds_for_waveforms(native, tmp_path, tool):
    from htk_amd import build as nbuild
    nbuild.build_tools()
    (tmp_path / "wav.conf").write_text("SOURCEFORMAT = WAV\nTARGETKIND = LPCEPSTRA\n")
    (tmp_path / "hmmlist").write_text("p0\n")
    (tmp_path / "dict").write_text("p0 p0\n")
    wav = os.path.join(GOLD, "test.wav")
    if tool == "herest":
        cmd = [os.path.join(BIN, "herest"), "-C", str(tmp_path / "wav.conf"), "-M", str(tmp_path), str(tmp_path / "hmmlist"), wav]
    else:
        cmd = [os.path.join(BIN, "hvite"), "-C", str(tmp_path / "wav.conf"), "-a", str(tmp_path / "dict"), str(tmp_path / "hmmlist"), wav]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "LPCEPSTRA" in r.stderr and "time-domain LPC kind" in r.stderr, r.stderr


# ---------------------------------------------------------------------------------------------------------------- on the device
@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(g.CASES))
def test_device_codes_the_golden_kinds_as_hcopy(native, case):
    cfg, kind = case_config(native, case)
    ref = golden(native, case)
    x, _ = native.wave_read(os.path.join(GOLD, "test.wav"))
    fe = native.FrontEnd(cfg)
    got, frameOff = fe.compute_host([x])
    fe.close()
    assert list(frameOff) == [0, ref.shape[0]]
    print("%s %s: %.4f of the values bit-equal, max |diff| %.3g" % (case, kind, bit_share(got, ref), np.abs(got - ref).max()))
    assert_matches(kind, got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("case", g.BATCH_CASES)
def test_device_codes_a_ragged_batch_as_hcopy(native, tmp_path, case):
    """8 waveforms of different lengths in one call: frame offsets per utterance, and every row as HCopy codes the file alone
    (committed in frontend_batch.npz; where oracle/_ref/HCopy is on the box it codes them live as well)."""
    cfg, kind = case_config(native, case)
    waves = g.batch_waves()
    z = np.load(os.path.join(GOLD, "frontend_batch.npz"))
    ref, refOff = z["batch_%s" % case], z["batch_%s_off" % case]
    if os.path.exists(HCOPY):
        live, liveOff = g.code_batch(HCOPY, case, waves, str(tmp_path))
        assert np.array_equal(live, ref) and np.array_equal(liveOff, refOff)
    fe = native.FrontEnd(cfg)
    got, frameOff = fe.compute_host(waves)
    fe.close()
    assert np.array_equal(frameOff, refOff)
    print("batch %s %s: %.4f of the values bit-equal" % (case, kind, bit_share(got, ref)))
    assert_matches(kind, got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ch", [("MFCC_0_D_A", 26), ("MFCC_E_D_A_Z", 40)])
def test_mfcc_through_the_frontend_is_the_mfcc_path(native, kind, ch):
    x, _ = native.wave_read(os.path.join(GOLD, "test.wav"))
    waves = [x] + g.batch_waves()
    a, offA = native.Mfcc(native.mfcc_config(kind, numChans=ch)).compute_host(waves)
    b, offB = native.FrontEnd(native.frontend_config(kind, numChans=ch)).compute_host(waves)
    assert np.array_equal(offA, offB) and np.array_equal(a, b)


@pytest.mark.gpu
def test_drivers_run_a_plp_recipe_from_waveforms(native, tmp_path):
    """herest / hvite with SOURCEFORMAT = WAV and TARGETKIND = PLP_0_D_A code test.wav on the device; one pass and one alignment give
    what the same tools give on the PLP_0_D_A file the reference's HCopy coded from it (tolerances of
    test_cli_tools.py::test_cli_tools_code_waveform_sources_on_the_device)."""
    from htk_amd import build as nbuild, synth
    nbuild.build_tools()
    s = synth.generate(12, 2, 4, 1, 98, 31, D=39)
    pk = s.packed()
    names = ["p%d" % i for i in range(pk["numPhys"])]
    synth.write_mmf_packed(str(tmp_path / "MMF"), pk, names, kind="PLP_0_D_A")
    (tmp_path / "hmmlist").write_text("\n".join(names) + "\n")
    (tmp_path / "wav.conf").write_text(open(os.path.join(GOLD, "frontend_a.conf")).read())
    (tmp_path / "plp.conf").write_text("TARGETKIND = PLP_0_D_A\n")
    (tmp_path / "dict").write_text("".join("%s %s\n" % (n, n) for n in names))
    lab = "\n".join(["p0", "p1", "p2", "p3", "p1"]) + "\n"
    outs = {}
    for tag, conf, data in (("wav", "wav.conf", os.path.join(GOLD, "test.wav")), ("plp", "plp.conf", os.path.join(GOLD, g.out_name("a")))):
        d = tmp_path / tag; d.mkdir()
        base = os.path.splitext(os.path.basename(data))[0]
        (d / (base + ".lab")).write_text(lab)
        r = subprocess.run([os.path.join(BIN, "herest"), "-C", str(tmp_path / conf), "-H", str(tmp_path / "MMF"), "-M", str(d), "-L", str(d),
                            "-m", "1", "-v", "0.01", str(tmp_path / "hmmlist"), data], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        lp = float(re.search(r"average log prob per frame = (\S+)", r.stdout).group(1))
        r2 = subprocess.run([os.path.join(BIN, "hvite"), "-C", str(tmp_path / conf), "-H", str(tmp_path / "MMF"), "-a", "-m", "-L", str(d),
                             "-l", str(d), "-y", "rec", str(tmp_path / "dict"), str(tmp_path / "hmmlist"), data],
                            capture_output=True, text=True, timeout=900)
        assert r2.returncode == 0, r2.stdout + r2.stderr
        outs[tag] = (lp, (d / (base + ".rec")).read_text().split())
    assert abs(outs["wav"][0] - outs["plp"][0]) <= 2e-6 * abs(outs["plp"][0])
    a, b = outs["wav"][1], outs["plp"][1]
    assert len(a) == len(b) and len(a) >= 15
    for x, y in zip(a, b):
        try:
            assert abs(float(x) - float(y)) <= 1e-3 * max(1.0, abs(float(y))), (x, y)
        except ValueError:
            assert x == y
