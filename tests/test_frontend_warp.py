"""VTLN frequency warping in the waveform front end (WARPFREQ / WARPLCUTOFF / WARPUCUTOFF: host/fbank.c, csrc/mfcc.hip,
htkamd_frontend_create_warped / _compute_warped / _compute_grid, capi.FrontEnd(warps=...), the drivers' waveform sources,
examples/vtln_warp.py) against the reference's HCopy.  The cases, their waveforms and the recipe of the committed rows are
tests/golden/make_frontend_warp_golden.py (frontend_warp.npz, frontend_warp.conf, test_MFCC_0_D_A.warp112.mfc)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "bin")
HCOPY = os.path.join(ROOT, "oracle", "_ref", "HCopy")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import make_frontend_warp_golden as wg  # noqa: E402
import make_wav_labels_golden as wl  # noqa: E402
from test_frontend_kinds import _VARS, assert_matches, bit_share  # noqa: E402

ALL = sorted(wg.CASES)
KINDS = ["mfcc26", "mfcc40", "fbank40", "melspec", "plp", "mfcc_ez"]          # all five factors each
_WARP_VARS = dict(_VARS, LOFREQ=("loFreq", float), HIFREQ=("hiFreq", float))
GOOD = (1.1, 300.0, 3400.0)


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(wg.NPZ)
    return {k: z[k] for k in z.files}, wg.read_confs()


@functools.lru_cache(maxsize=None)
def waves(case):
    return tuple(wg.case_waves(case))


def case_kw(case):
    """(TARGETKIND, keyword arguments of frontend_config) of `case` from its committed configuration text; the period is the WAV
    header's as the reference forms it (HWave.c:1107)."""
    kw, kind = {"usePower": False, "eNormalise": True, "numChans": 20, "sampPeriod": 1.0e7 / wg.CASES[case][0]}, None
    for line in fixture()[1][case].splitlines():
        k, v = (x.strip() for x in line.split("="))
        if k == "TARGETKIND":
            kind = v
        elif k in _WARP_VARS:
            name, typ = _WARP_VARS[k]
            kw[name] = (v[0] in "Tt") if typ == "bool" else typ(v)
        else:
            assert k == "SOURCEFORMAT" and v == "WAV", line
    return kind, kw


def create_warped(native, cfg, warps):
    """(return code, error string) of htkamd_frontend_create_warped; a handle it made is destroyed"""
    arr = (native.Warp * max(len(warps), 1))(*[native.Warp(*w) for w in warps])
    h = C.c_void_p()
    rc = native.lib().htkamd_frontend_create_warped(C.byref(cfg), arr, C.c_int(len(warps)), C.byref(h))
    if rc == 0:
        native.lib().htkamd_frontend_destroy(h)
    return rc, native.lib().htkamd_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- host only
def test_fixture_holds_every_case_of_the_recipe():
    rows, confs = fixture()
    assert sorted(confs) == ALL
    assert sorted(rows) == sorted([wg.key(c, a) for c in ALL for a in wg.CASES[c][5]] + [c + "_off" for c in ALL])
    for case in ALL:
        assert confs[case] == wg.conf_text(case), case
        assert 1.0 in wg.CASES[case][5]
        for a in wg.CASES[case][5]:
            r = rows[wg.key(case, a)]
            assert list(np.diff(rows[case + "_off"])) == list(wg.CASES[case][6]) and r.shape[0] == rows[case + "_off"][-1]
            if a != 1.0:                                          # a fixture in which the warp has no effect proves nothing
                assert np.abs(r - rows[wg.key(case, 1.0)]).max() > 1e-3, (case, a)
    assert os.path.getsize(wg.NPZ) < os.path.getsize(os.path.join(wg.OUT, "frontend_batch.npz"))
    assert sum(wg.CASES["ragged"][6][:3]) % 2 == 0 and wg.CASES["ragged"][6][0] % 2 == 1      # two utterances in one pair of frames


def test_capi_exposes_the_warp_entry_points(native):
    for name in ("htkamd_frontend_create_warped", "htkamd_frontend_num_warps", "htkamd_frontend_compute_warped", "htkamd_frontend_compute_grid"):
        assert hasattr(native.lib(), name), name
    assert C.sizeof(native.Warp) == 12
    for name in ("compute_grid", "compute_grid_host", "compute", "compute_host"):
        assert hasattr(native.FrontEnd, name)
    assert native.lib().htkamd_frontend_num_warps(None) == 0


@pytest.mark.parametrize("kw,warp,why", [
    ({}, (0.49, 300.0, 3400.0), "unlikely warping factor WARPFREQ 0.49"),
    ({}, (2.01, 300.0, 3400.0), "unlikely warping factor WARPFREQ 2.01"),
    ({}, (1.1, 0.0, 3400.0), "invalid warping cut-off frequencies WARPLCUTOFF 0 WARPUCUTOFF 3400"),
    ({}, (1.1, 300.0, 0.0), "invalid warping cut-off frequencies WARPLCUTOFF 300 WARPUCUTOFF 0"),
    ({}, (0.9, 3400.0, 300.0), "invalid warping cut-off frequencies WARPLCUTOFF 3400 WARPUCUTOFF 300"),
    ({"loFreq": 400.0}, (1.1, 300.0, 3400.0), "does not lie above the band's lower end"),          # cl <= minFreq
    ({}, (1.1, 300.0, 8000.0), "does not lie below the band's upper end"),                         # cu >= maxFreq
    ({"hiFreq": 3600.0}, (0.88, 300.0, 3400.0), "at or beyond the band's upper end"),              # scale * cu >= maxFreq
    ({"loFreq": 300.0}, (1.3, 310.0, 3400.0), "at or below the band's lower end"),                 # scale * cl <= minFreq
])
def test_refused_warps(native, kw, warp, why):
    """Refusals come with their reason and before the device is looked for (as test_frontend_kinds.test_refused_configurations)."""
    cfg = native.frontend_config("MFCC_0_D_A", **kw)
    for warps in ([warp], [GOOD, warp]):
        rc, err = create_warped(native, cfg, warps)
        assert rc == -1 and why in err, (rc, err)


def test_refused_warp_counts_and_arguments(native):
    cfg = native.frontend_config("MFCC_0_D_A")
    for n in (0, 65):
        rc, err = create_warped(native, cfg, [GOOD] * n)
        assert rc == -1 and "%d warps (1..64)" % n in err, (rc, err)
    h = C.c_void_p()
    assert native.lib().htkamd_frontend_create_warped(C.byref(cfg), None, C.c_int(1), C.byref(h)) == -1
    # a refused configuration is refused with its own reason, whatever the warp
    rc, err = create_warped(native, native.frontend_config("FBANK_0"), [GOOD])
    assert rc == -1 and "_0 on FBANK" in err
    # an un-warped triple needs no cut-offs; a good one passes the checks: what is left to fail without a device is the device
    for warps in ([(1.0, 0.0, 0.0)], [GOOD] * 64):
        rc, err = create_warped(native, cfg, warps)
        assert rc == 0 or (native.lib().htkamd_device_count() <= 0 and "no HIP device" in err), (rc, err)


def test_warped_host_tables_of_every_case_under_sanitizers(native, tmp_path):
    """fbank.c's warped table builder under AddressSanitizer + UndefinedBehaviorSanitizer through a stand-alone program with the
    sanitizers' runtimes linked in (tests/frontend_warp_sanitize.c), every case and factor of the fixture: the filters' edges increase
    strictly, every loWt lies in [0, 1], and the tables of warpFreq 1.0 are the un-warped ones byte for byte."""
    asan = subprocess.run(["gcc", "-print-file-name=libasan.a"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no static libasan in this toolchain")
    lines = []
    for case in ALL:
        kind, kw = case_kw(case)
        c = native.frontend_config(kind, **kw)
        b = c.base
        for w in wg.warps(case) + [(1.0, 0.0, 0.0)]:
            lines.append("%s_%g %d %r %r %r %d %d %d %d %r %r %d %r %r %r %r" % (
                case, w[0], c.baseKind, b.sampPeriod, b.winDur, b.frPeriod, b.numChans, b.numCeps, b.cepLifter, b.usePower, b.loFreq, b.hiFreq,
                c.lpcOrder, c.compressFact, w[0], w[1], w[2]))
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "frontend_warp_sanitize")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "frontend_warp_sanitize.c"),
                           os.path.join(ROOT, "htk_amd", "host", "fbank.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(tmp_path / "cases.txt")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "OK %d" % len(lines), (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("tool", ["herest", "hvite"])
def test_drivers_refuse_a_warp_without_cut_offs(native, tmp_path, tool):
    from htk_amd import build as nbuild
    nbuild.build_tools()
    (tmp_path / "wav.conf").write_text("SOURCEFORMAT = WAV\nTARGETKIND = MFCC_0_D_A\nWARPFREQ = 1.1\n")
    (tmp_path / "hmmlist").write_text("p0\n")
    (tmp_path / "dict").write_text("p0 p0\n")
    wav = wg.WAV
    if tool == "herest":
        cmd = [os.path.join(BIN, "herest"), "-C", str(tmp_path / "wav.conf"), "-M", str(tmp_path), str(tmp_path / "hmmlist"), wav]
    else:
        cmd = [os.path.join(BIN, "hvite"), "-C", str(tmp_path / "wav.conf"), "-a", str(tmp_path / "dict"), str(tmp_path / "hmmlist"), wav]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "invalid warping cut-off frequencies WARPLCUTOFF 0 WARPUCUTOFF 0" in r.stderr, r.stderr


# ---------------------------------------------------------------------------------------------------------------- on the device
@functools.lru_cache(maxsize=None)
def single_warp_rows(native, case):
    """the case's batch coded by one single-warp front end per factor (compute_warped, every utterance on warp 0): factor -> rows"""
    kind, kw = case_kw(case)
    out = {}
    for w in wg.warps(case):
        fe = native.FrontEnd(native.frontend_config(kind, **kw), warps=[w])
        assert fe.num_warps == 1
        got, off = fe.compute_host(list(waves(case)), warp_index=[0] * len(waves(case)))
        fe.close()
        assert np.array_equal(off, fixture()[0][case + "_off"])
        got.setflags(write=False)
        out[w[0]] = got
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL)
def test_device_codes_every_warped_case_as_hcopy(native, tmp_path, case):
    """compute_warped on every case and factor against HCopy's rows, by the rule of test_frontend_kinds.assert_matches; where
    oracle/_ref/HCopy is on the box it codes the batches live as well."""
    kind, _ = case_kw(case)
    rows = fixture()[0]
    got = single_warp_rows(native, case)
    for alpha in wg.CASES[case][5]:
        ref = rows[wg.key(case, alpha)]
        if os.path.exists(HCOPY):
            live, liveOff = wg.code_batch(HCOPY, case, alpha, waves(case), str(tmp_path))
            assert np.array_equal(live, ref) and np.array_equal(liveOff, rows[case + "_off"])
        print("warp %s %s alpha %.2f: %.4f of the values bit-equal to HCopy, max |diff| %.3g"
              % (case, kind, alpha, bit_share(got[alpha], ref), np.abs(got[alpha] - ref).max()))
    for alpha in wg.CASES[case][5]:
        assert_matches(kind, got[alpha], rows[wg.key(case, alpha)])


@pytest.mark.gpu
def test_unwarped_calls_on_a_warped_handle(native):
    """htkamd_frontend_compute on a warped handle codes with warps[0]; warpFreq 1.0 is the un-warped front end; a warp index outside
    the handle's warps is refused."""
    case = "mfcc26"
    kind, kw = case_kw(case)
    cfg, ws = native.frontend_config(kind, **kw), wg.warps(case)
    single = single_warp_rows(native, case)
    fe = native.FrontEnd(cfg, warps=ws)
    assert fe.num_warps == len(ws)
    assert np.array_equal(fe.compute_host(list(waves(case)))[0], single[ws[0][0]])
    with pytest.raises(native.HtkAmdError, match="asks for warp 5 of 5"):
        fe.compute_host(list(waves(case)), warp_index=[0, 1, 5, 2])
    with pytest.raises(native.HtkAmdError, match="asks for warp -1 of 5"):
        fe.compute_host(list(waves(case)), warp_index=[0, -1, 0, 0])
    fe.close()
    plain = native.FrontEnd(cfg)
    assert plain.num_warps == 1
    assert np.array_equal(plain.compute_host(list(waves(case)))[0], single[1.0])
    plain.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ragged", "mfcc40", "plp"])
def test_every_utterance_under_its_own_warp(native, case):
    """One call with a different warp for each neighbouring utterance is, utterance by utterance, what single-warp batches give (and
    so matches HCopy): in `ragged` the utterances of 1, 2 and 3 frames put two warps into one pair of frames."""
    kind, kw = case_kw(case)
    ws, off = wg.warps(case), fixture()[0][case + "_off"]
    single = single_warp_rows(native, case)
    fe = native.FrontEnd(native.frontend_config(kind, **kw), warps=ws)
    for shift in (0, 2):
        idx = [(u + shift) % len(ws) for u in range(len(off) - 1)]
        got, gotOff = fe.compute_host(list(waves(case)), warp_index=idx)
        assert np.array_equal(gotOff, off)
        for u, w in enumerate(idx):
            assert np.array_equal(got[off[u]:off[u + 1]], single[ws[w][0]][off[u]:off[u + 1]]), (case, shift, u, w)
            assert_matches(kind, got[off[u]:off[u + 1]], fixture()[0][wg.key(case, ws[w][0])][off[u]:off[u + 1]])
    fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", KINDS + ["fft128", "ragged"])
def test_grid_tables_are_the_single_warp_tables(native, case):
    """compute_grid's table w is compute_warped with every utterance on warp w, every float: the same device arithmetic."""
    kind, kw = case_kw(case)
    ws = wg.warps(case)
    single = single_warp_rows(native, case)
    fe = native.FrontEnd(native.frontend_config(kind, **kw), warps=ws)
    grid, off = fe.compute_grid_host(list(waves(case)))
    assert np.array_equal(off, fixture()[0][case + "_off"]) and grid.shape[0] == len(ws)
    for w, warp in enumerate(ws):
        assert np.array_equal(grid[w], single[warp[0]]), (case, warp[0], int((grid[w] != single[warp[0]]).sum()))
        assert np.array_equal(fe.compute_host(list(waves(case)), warp_index=[w] * (len(off) - 1))[0], single[warp[0]])
    fe.close()


@pytest.mark.gpu
def test_hvite_aligns_a_warped_wav_as_the_hcopy_coded_file(native, tmp_path):
    """hvite -a on test.wav with WARPFREQ = 1.12 writes the label file it writes on the parameter file HCopy coded from test.wav with
    that configuration; with WARPFREQ = 1.0 the scores are others."""
    from htk_amd import build as nbuild
    nbuild.build_tools()
    d = str(tmp_path)
    wl.write_case(d)
    (tmp_path / "parm.conf").write_text("TARGETKIND = MFCC_0_D_A\n")
    recs = {}
    for tag, conf, data in (("warped", wg.wav_conf(wg.WAV_WARP[0]), wg.WAV), ("plain", wg.wav_conf(1.0), wg.WAV), ("parm", None, wg.WAV_PARM)):
        out = tmp_path / tag
        out.mkdir()
        if conf:
            (out / "conf").write_text(conf)
        base = os.path.splitext(os.path.basename(data))[0]
        (out / (base + ".lab")).write_text("\n".join(wl.LABELS) + "\n")
        r = subprocess.run([os.path.join(BIN, "hvite"), "-C", str(out / "conf") if conf else str(tmp_path / "parm.conf"), "-H", os.path.join(d, "MMF"),
                            "-l", str(out), "-y", "rec", "-a", "-m", "-f", "-L", str(out), os.path.join(d, "dict"), os.path.join(d, "hmmlist"), data],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        recs[tag] = (out / (base + ".rec")).read_text()
    assert len(recs["parm"].splitlines()) >= 15
    assert recs["warped"] == recs["parm"]
    assert recs["plain"] != recs["parm"]


@pytest.mark.gpu
def test_example_picks_the_same_factors_from_the_grid_as_from_single_runs(native):
    """examples/vtln_warp.py on a tiny set (the ragged case's three longest utterances, two speakers, the set fitted to test.wav): per
    speaker the same factor from one compute_grid call as from one single-warp run per factor, from the same scores."""
    import vtln_warp
    case = "ragged"
    kind, kw = case_kw(case)
    ws = wg.warps(case)
    batch = list(waves(case))[2:]
    speakers = ["a", "b", "a"]
    mmf = native.Mmf([os.path.join(wg.OUT, "fitted.mmf")])
    model = native.Model(mmf.packed())
    seqs = [[0], [1, 2], [0, 1, 2, 3, 4]]
    labOff = np.concatenate([[0], np.cumsum([len(q) for q in seqs])]).astype(np.int32)
    labs = np.concatenate(seqs).astype(np.int32)
    cfg = native.frontend_config(kind, **kw)
    best, scores = vtln_warp.pick_warps(cfg, batch, speakers, model, labOff, labs, ws, grid=True)
    best1, scores1 = vtln_warp.pick_warps(cfg, batch, speakers, model, labOff, labs, ws, grid=False)
    assert np.isfinite(scores).all() and len(set(scores[:, 2])) == len(ws)
    assert np.array_equal(scores, scores1)
    assert best == best1 and sorted(best) == ["a", "b"]


@pytest.mark.gpu
def test_example_runs_end_to_end_on_the_committed_wav(native, tmp_path):
    """examples/vtln_warp.py as a user runs it: configuration file, script file with speakers, label files beside the waveforms, the
    factors' range; the `speaker alpha` lines name factors of the grid, and the recoded batch is every file under its speaker's factor."""
    import shutil
    import vtln_warp
    names = wl.write_case(str(tmp_path))
    (tmp_path / "front.conf").write_text("# front end\nSOURCEFORMAT = WAV\n" + wl.FRONT + "HPARM: TARGETKIND = MFCC_0_D_A\n")
    x, _ = native.wave_read(wg.WAV)
    files = []
    for i, spk in enumerate(("anna", "ben")):
        f = tmp_path / ("u%d.wav" % i)
        if i == 0:
            shutil.copy(wg.WAV, f)
        else:                                                     # another waveform: the same speech, louder and with an offset
            wg.write_wav(str(f), (x.astype(np.int32) * 3 // 2 + 40).clip(-32768, 32767), 16000)
        (tmp_path / ("u%d.lab" % i)).write_text("\n".join(names) + "\n")
        files.append((str(f), spk))
    (tmp_path / "files.scp").write_text("".join("%s %s\n" % fs for fs in files))
    best = vtln_warp.main(["-C", str(tmp_path / "front.conf"), "-H", str(tmp_path / "MMF"), "--scp", str(tmp_path / "files.scp"),
                           "--factors", "0.94:1.06:3", "-o", str(tmp_path / "warps.txt"), "--features", str(tmp_path / "feats.npz"),
                           str(tmp_path / "hmmlist")])
    factors = [0.94, 1.0, 1.06]
    lines = [l.split() for l in (tmp_path / "warps.txt").read_text().splitlines()]
    assert [l[0] for l in lines] == ["anna", "ben"] and all(float(l[1]) in factors for l in lines)
    assert [factors[best[s]] for s in ("anna", "ben")] == [float(l[1]) for l in lines]
    z = np.load(str(tmp_path / "feats.npz"))
    assert list(z["frameOff"]) == [0, 98, 196] and z["feats"].shape == (196, 39)
    kind, kw = vtln_warp.read_config(str(tmp_path / "front.conf"))
    assert kind == "MFCC_0_D_A" and kw["sampPeriod"] == 625.0 and kw["eNormalise"] is False
    for i, (f, spk) in enumerate(files):
        fe = native.FrontEnd(native.frontend_config(kind, **kw), warps=[(factors[best[spk]], 300.0, 3400.0)])
        one, _ = fe.compute_host([native.wave_read(f)[0]])
        fe.close()
        assert np.array_equal(z["feats"][98 * i:98 * (i + 1)], one)
