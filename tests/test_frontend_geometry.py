"""The waveform front end (csrc/mfcc.hip, host/fbank.c, oracle/orc_mfcc.c) away from 16 kHz / 25 ms, against the reference's HCopy:
every FFT size from 8 to 4096 points (stage pairs alone, a lone last stage, fewer work items than lanes), windows with no and with
almost all zero padding, sample periods that are no whole number of 100 ns units, the lane layouts on either side of the
two-frames-per-wavefront limits, channel counts beyond one wavefront, and regression windows 3 / 1 on utterances of 1, 2 and 3 frames.
The cases, their waveforms and the recipe of the committed rows are tests/golden/make_frontend_geom_golden.py (frontend_geom.npz,
frontend_geom.conf)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HCOPY = os.path.join(ROOT, "oracle", "_ref", "HCopy")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_frontend_geom_golden as gg  # noqa: E402
from test_frontend_kinds import _VARS, assert_matches, bit_share  # noqa: E402

ALL = sorted(gg.CASES)
MFCC = [c for c in ALL if gg.CASES[c][1].startswith("MFCC")]
_GEOM_VARS = dict(_VARS, LOFREQ=("loFreq", float), HIFREQ=("hiFreq", float), DELTAWINDOW=("delWin", int), ACCWINDOW=("accWin", int))


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(gg.NPZ)
    return {k: z[k] for k in z.files}, gg.read_confs()


@functools.lru_cache(maxsize=None)
def waves(case):
    return tuple(gg.case_waves(case))


def case_kw(case):
    """(TARGETKIND, keyword arguments of frontend_config / mfcc_cfg) of `case` from its committed configuration text: HParm's defaults
    for what it does not set, and -- there is no SOURCERATE -- the period of the WAV header as the reference forms it (HWave.c:1107)."""
    kw, kind = {"usePower": False, "eNormalise": True, "numChans": 20, "sampPeriod": 1.0e7 / gg.rate(case)}, None
    for line in fixture()[1][case].splitlines():
        k, v = (x.strip() for x in line.split("="))
        if k == "TARGETKIND":
            kind = v
        elif k in _GEOM_VARS:
            name, typ = _GEOM_VARS[k]
            kw[name] = (v[0] in "Tt") if typ == "bool" else typ(v)
        else:
            assert k == "SOURCEFORMAT" and v == "WAV", line
    return kind, kw


def oracle_rows(oracle, case):
    kind, kw = case_kw(case)
    cfg = oracle.mfcc_cfg(kind, **kw)
    return np.concatenate([oracle.mfcc(w, cfg) for w in waves(case)])


# ---------------------------------------------------------------------------------------------------------------- host only
def test_fixture_holds_every_case_of_the_recipe():
    rows, confs = fixture()
    assert sorted(confs) == ALL and sorted(rows) == sorted(ALL + [c + "_off" for c in ALL])
    for case in ALL:
        assert confs[case] == gg.conf_text(case), case
        assert "SOURCERATE" not in confs[case]
        assert list(np.diff(rows[case + "_off"])) == list(gg.CASES[case][3]) and rows[case].shape[0] == rows[case + "_off"][-1]
    # what the cases are there for: every FFT size, and an odd number of frames for the paired kernel's last wavefront
    assert sorted({g[4] for g in gg.GEOMS.values()}) == [8, 128, 256, 512, 1024, 2048, 4096]
    assert all(sum(c[3]) % 2 == 1 for c in gg.CASES.values())


@pytest.mark.parametrize("case", MFCC)
def test_oracle_codes_every_geometry_as_hcopy(oracle, case):
    """oracle.mfcc against the reference's HCopy, every float: at 22.05, 44.1 and 48 kHz only with InitFBank's period truncated to a
    long as the reference truncates it (HParm.c:2167, HSigP.c:471)."""
    ref = fixture()[0][case]
    got = oracle_rows(oracle, case)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), "%d of %d values differ, max %.3g" % ((got != ref).sum(), got.size, np.abs(got - ref).max())


@pytest.mark.parametrize("case", ALL)
def test_frame_and_column_counts_are_hcopys(native, case):
    kind, kw = case_kw(case)
    cfg = native.frontend_config(kind, **kw)
    rows = fixture()[0]
    frames = [native.lib().htkamd_frontend_num_frames(C.byref(cfg), C.c_int(len(w))) for w in waves(case)]
    assert frames == list(np.diff(rows[case + "_off"]))
    assert native.frontend_num_cols(cfg) == rows[case].shape[1]
    t = native.lib().htkamd_frontend_num_frames
    frSize = gg.GEOMS[gg.CASES[case][0]][3]
    assert t(C.byref(cfg), C.c_int(frSize)) == 1 and t(C.byref(cfg), C.c_int(frSize - 1)) == 0


@pytest.mark.parametrize("hz", sorted({g[0] for g in gg.GEOMS.values()}))
def test_wav_header_period_is_the_references_double(native, tmp_path, hz):
    """HWave.c:1107 divides the double 1.0E7 by the rate: at 44.1 kHz a 10 ms shift is 441 samples, with a float quotient 440."""
    path = str(tmp_path / "x.wav")
    gg.write_wav(path, np.zeros(16, np.int16), hz)
    _, per = native.wave_read(path)
    assert per == 1.0e7 / hz
    for g in gg.GEOMS.values():
        if g[0] == hz:
            assert int(g[1] / per) == g[3]


def test_host_tables_of_every_case_under_sanitizers(native, tmp_path):
    """fbank.c's validation and table builder and the oracle's restatement under AddressSanitizer + UndefinedBehaviorSanitizer, every
    case's configuration, through a stand-alone program with the sanitizers' runtimes linked in (tests/frontend_geom_sanitize.c): the 8- and the 4096-point rows are where a
    table one element short would show."""
    asan = subprocess.run(["gcc", "-print-file-name=libasan.a"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no static libasan in this toolchain")
    lines = []
    for case in ALL:
        kind, kw = case_kw(case)
        c = native.frontend_config(kind, **kw)
        b = c.base
        lines.append("%s %d %r %r %r %d %d %d %r %d %d %d %d %d %r %r %d %d %d %d %d %d %d %d %r %d" % (
            case, c.baseKind, b.sampPeriod, b.winDur, b.frPeriod, b.numChans, b.numCeps, b.cepLifter, b.preEmph, b.useHam, b.usePower,
            b.zMeanSource, b.rawEnergy, b.eNormalise, b.loFreq, b.hiFreq, b.hasC0, b.hasE, b.hasD, b.hasA, b.hasZ, b.delWin, b.accWin,
            c.lpcOrder, c.compressFact, len(waves(case)[-1])))
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "frontend_geom_sanitize")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "frontend_geom_sanitize.c"),
                           os.path.join(ROOT, "htk_amd", "host", "fbank.c"), os.path.join(ROOT, "oracle", "orc_mfcc.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(tmp_path / "cases.txt")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "OK %d" % len(ALL), (r.stdout[-2000:], r.stderr[-4000:])


# ---------------------------------------------------------------------------------------------------------------- on the device
@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL)
def test_device_codes_every_geometry_as_hcopy(native, oracle, tmp_path, case):
    """One compute_host per case: the frame offsets are the fixture's; FBANK, MELSPEC and PLP rows match HCopy's by the rule of
    test_frontend_kinds.assert_matches; MFCC rows equal the oracle's bit for bit (the contract of test_mfcc_matches_reference_front_end)
    and match HCopy's by the same rule.  Where oracle/_ref/HCopy is on the box it codes the batch live as well."""
    kind, kw = case_kw(case)
    rows = fixture()[0]
    ref, refOff = rows[case], rows[case + "_off"]
    if os.path.exists(HCOPY):
        live, liveOff = gg.code_batch(HCOPY, case, waves(case), str(tmp_path))
        assert np.array_equal(live, ref) and np.array_equal(liveOff, refOff)
    fe = native.FrontEnd(native.frontend_config(kind, **kw))
    got, frameOff = fe.compute_host(list(waves(case)))
    fe.close()
    assert np.array_equal(frameOff, refOff)
    assert got.shape == ref.shape
    print("geom %s %s: %.4f of the values bit-equal to HCopy, max |diff| %.3g" % (case, kind, bit_share(got, ref), np.abs(got - ref).max()))
    if kind.startswith("MFCC"):
        orc = oracle_rows(oracle, case)
        print("geom %s %s: %.4f of the values bit-equal to the oracle" % (case, kind, bit_share(got, orc)))
        assert np.array_equal(got, orc), "%d of %d values differ, max %.3g" % ((got != orc).sum(), got.size, np.abs(got - orc).max())
    assert_matches(kind, got, ref)
