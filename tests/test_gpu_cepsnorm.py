"""Side-based cepstral mean and variance normalisation on the device (htk_amd/csrc/cepsnorm.hip): htkamd_side_stats against fp64
NumPy and against the side files the reference's HCompV wrote, htkamd_parm_normalise against the files the reference's HCopy wrote
(tests/golden/cmvn, make_cmvn_golden.py), and the drivers with the CMEAN* / VARSCALE* configuration.

The bar against HCompV's files: make_cmvn_golden.py measured the reference's own deviation from fp64 arithmetic on these fixtures (its
float sums per utterance and side, plus the 7 digits of %e) as 5.72e-07 of a standard deviation for the means and 2.96e-06 relative for
the variances; the device (fp64 sums, rounded once) has to be within 4 x that of the reference's files."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "cmvn")
BIN = os.path.join(ROOT, "tools", "bin")
REF_DEV_MEAN, REF_DEV_VAR = 5.72e-07, 2.96e-06
MIXED = ["spb_1", "spa_1", "tpc_1", "spa_2", "spb_2", "spa_3"]          # one batch, the sides interleaved
SIDES = ["spa", "spb", "tpc"]
LENS = [1, 2, 63, 64, 65, 127, 128, 129, 300]
UTT_SIDE = [2, 0, 3, 2, 0, 0, 3, 2, 0]                                   # 4 sides dealt out of order, side 1 left empty


def case_conf(case):
    return dict(l.split(" = ") for l in open(os.path.join(GOLD, case + ".conf")).read().replace("@GOLD@", GOLD).splitlines())


def side_file(native, conf, prefix, name):
    """<DIR>/[<path mask's capture>/]<mask's capture> for data/<name>.mfc"""
    fn = os.path.join(GOLD, "data", name + ".mfc")
    parts = [conf[prefix + "DIR"]]
    if prefix + "PATHMASK" in conf:
        parts.append(native.mask_match(conf[prefix + "PATHMASK"], fn))
    return os.path.join(*parts, native.mask_match(conf[prefix + "MASK"], fn))


@pytest.fixture(scope="module")
def coded(native):
    """The six fixture files as MFCC_E_D_A on the device (the qualifier step without _Z), in the MIXED order."""
    stat = [native.parm_read(os.path.join(GOLD, "data", n + ".mfc"))[0] for n in MIXED]
    dX, frameOff, cols = native.parm_qualify(stat, native.parm_quals_from_kind("MFCC_E_D_A", 13))
    assert cols == 39
    host = dX.to_host(np.float32, (int(frameOff[-1]), cols))
    return host, frameOff


@pytest.mark.parametrize("nCols,D", [(39, 39), (39, 13), (120, 120)])
def test_side_statistics_against_fp64_numpy(native, nCols, D):
    rng = np.random.default_rng(nCols * 1000 + D)
    X = (rng.normal(0.0, 3.0, (sum(LENS), nCols)) + rng.uniform(5, 20, nCols) * rng.choice([-1.0, 1.0], nCols)).astype(np.float32)      # column means away from 0: the sums are well conditioned
    frameOff = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    dX = native.DevArray(X)
    s, q, n = native.side_stats(dX.ptr, frameOff, UTT_SIDE, 4, nCols, D)
    s2, q2, n2 = native.side_stats(dX.ptr, frameOff, UTT_SIDE, 4, nCols, D)
    assert s.tobytes() == s2.tobytes() and q.tobytes() == q2.tobytes() and np.array_equal(n, n2)      # the same bits on every call
    for side in range(4):
        rows = np.concatenate([X[frameOff[u]:frameOff[u + 1], :D] for u in range(len(LENS)) if UTT_SIDE[u] == side] or [np.zeros((0, D), np.float32)]).astype(np.float64)
        assert n[side] == rows.shape[0]
        rs, rq = rows.sum(0), (rows * rows).sum(0)
        if side == 1:
            assert n[side] == 0 and not s[side].any() and not q[side].any()
            continue
        errS = np.max(np.abs(s[side] - rs) / np.abs(rs)); errQ = np.max(np.abs(q[side] - rq) / rq)
        print("side %d: sums %.3g, squares %.3g relative" % (side, errS, errQ))
        assert errS <= 1e-12 and errQ <= 1e-12                        # only the order of the fp64 additions differs
    mean, var = native.side_stats_finish(s, q, n)
    assert not mean[1].any() and not var[1].any()


def test_side_statistics_against_the_reference_files(native, coded):
    """Within 4 x the reference's own measured deviation from fp64 arithmetic (module docstring; tests/golden/cmvn/README)."""
    readme = open(os.path.join(GOLD, "README")).read()
    assert "%.3g" % REF_DEV_MEAN in readme and "%.3g" % REF_DEV_VAR in readme
    host, frameOff = coded
    uttSide = [SIDES.index(n[:3]) for n in MIXED]
    dX = native.DevArray(host)
    s, q, n = native.side_stats(dX.ptr, frameOff, uttSide, 3, 39, 39)
    mean, var = native.side_stats_finish(s, q, n)
    for i, side in enumerate(SIDES):
        ref = native.cepsnorm_read(os.path.join(GOLD, "cmn", side))
        assert n[i] == ref["nFrames"]
        devM = np.max(np.abs(mean[i].astype(np.float64) - ref["mean"]) / np.sqrt(ref["var"].astype(np.float64)))
        devV = np.max(np.abs(var[i].astype(np.float64) - ref["var"]) / ref["var"])
        print("%s: means %.3g of a standard deviation, variances %.3g relative" % (side, devM, devV))
        assert devM <= 4 * REF_DEV_MEAN and devV <= 4 * REF_DEV_VAR


@pytest.mark.parametrize("case", ["mean", "var", "both", "path"])
def test_normalised_table_is_hcopys(native, coded, case):
    """The qualifier step is bit-equal to the reference already; behind it come one float subtraction and one float multiplication by
    host-built constants, so the device's table equals HCopy's file in every value."""
    conf = case_conf(case)
    host, frameOff = coded
    means = scale = None
    fileSides = []
    keys = []
    for name in MIXED:
        key = (side_file(native, conf, "CMEAN", name) if "CMEANDIR" in conf else "", side_file(native, conf, "VARSCALE", name) if "VARSCALEDIR" in conf else "")
        if key not in keys:
            keys.append(key)
        fileSides.append(keys.index(key))
    assert len(keys) == 3
    target = native.parm_kind_parse(conf["TARGETKIND"])
    if "CMEANDIR" in conf:
        files = [native.cepsnorm_read(k[0]) for k in keys]
        for f in files:
            native.cepsnorm_check_kinds(target, f["kind"], -1)
        means = np.stack([f["mean"] for f in files])
    if "VARSCALEDIR" in conf:
        files = [native.cepsnorm_read(k[1]) for k in keys]
        for f in files:
            native.cepsnorm_check_kinds(target, -1, f["kind"])
        scale = native.cepsnorm_scale(native.varscale_read(conf["VARSCALEFN"]), np.stack([f["var"] for f in files]), [k[1] for k in keys])
    dX = native.DevArray(host)
    native.parm_normalise(dX.ptr, frameOff, fileSides, 3, 39, mean=means, scale=scale)
    got = dX.to_host(np.float32, host.shape)
    ref = []
    for name in MIXED:
        # (under path.conf HCopy wrote the bytes of out/mean -- make_cmvn_golden.py checks it -- so those files are kept once)
        x, _, kind = native.parm_read(os.path.join(GOLD, "out", "mean" if case == "path" else case, name + ".htk"))
        assert native.parm_kind_str(kind) == conf["TARGETKIND"]
        ref.append(x)
    ref = np.concatenate(ref)
    assert got.shape == ref.shape
    print("%s: %d of %d values differ" % (case, int((got != ref).sum()), ref.size))
    assert np.array_equal(got, ref)
    if case == "mean":                                                 # only the leading dMean columns are touched: a 13-column mean
        dY = native.DevArray(host)
        native.parm_normalise(dY.ptr, frameOff, fileSides, 3, 39, mean=means[:, :13])
        part = dY.to_host(np.float32, host.shape)
        assert np.array_equal(part[:, :13], ref[:, :13]) and np.array_equal(part[:, 13:], host[:, 13:])


def test_side_out_of_range_is_refused(native, coded):
    host, frameOff = coded
    dX = native.DevArray(host)
    for bad in (3, -1):
        with pytest.raises(native.HtkAmdError) as e:
            native.parm_normalise(dX.ptr, frameOff, [0, 1, 2, bad, 1, 0], 3, 39, mean=np.ones((3, 39), np.float32))
        assert e.value.rc == -1 and "side %d of 3" % bad in str(e.value)
        with pytest.raises(native.HtkAmdError) as e:
            native.side_stats(dX.ptr, frameOff, [0, 1, 2, bad, 1, 0], 3, 39, 39)
        assert e.value.rc == -1
    assert np.array_equal(dX.to_host(np.float32, host.shape), host)    # refused before anything was launched


def test_drivers_normalise_as_hcopy_did(native, tmp_path):
    """herest and hvite -a with the CMEAN* / VARSCALE* configuration on the raw files give what they give with a plain configuration
    on the files HCopy normalised: the same log probability, the same re-estimated models byte for byte, the same label files.  A mask
    that does not match ends the run with the mask named."""
    from htk_amd import build as nbuild, synth
    nbuild.build_tools()
    s = synth.generate(12, 2, 4, 1, 98, 31, D=39)
    pk = s.packed()
    names = ["p%d" % i for i in range(pk["numPhys"])]
    synth.write_mmf_packed(str(tmp_path / "MMF"), pk, names, kind="MFCC_E_D_A_Z")
    (tmp_path / "hmmlist").write_text("\n".join(names) + "\n")
    both = open(os.path.join(GOLD, "both.conf")).read().replace("@GOLD@", GOLD)
    (tmp_path / "side.conf").write_text(both)
    (tmp_path / "plain.conf").write_text("TARGETKIND = MFCC_E_D_A_Z\n")
    (tmp_path / "wrong.conf").write_text(both.replace("CMEANMASK = */%%%_*.mfc", "CMEANMASK = */%%%-*.mfc"))
    (tmp_path / "dict").write_text("".join("%s %s\n" % (n, n) for n in names))
    lab = "\n".join(["p0", "p1", "p2", "p3", "p1"]) + "\n"
    use = ["spa_1", "tpc_1", "spb_2"]
    outs = {}
    for tag, conf, data in (("side", "side.conf", [os.path.join(GOLD, "data", n + ".mfc") for n in use]),
                            ("plain", "plain.conf", [os.path.join(GOLD, "out", "both", n + ".htk") for n in use])):
        d = tmp_path / tag; d.mkdir()
        for n in use:
            (d / (n + ".lab")).write_text(lab)
        r = subprocess.run([os.path.join(BIN, "herest"), "-C", str(tmp_path / conf), "-H", str(tmp_path / "MMF"), "-M", str(d), "-L", str(d),
                            "-m", "1", "-v", "0.01", str(tmp_path / "hmmlist")] + data, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        lp = re.search(r"average log prob per frame = (\S+)", r.stdout).group(1)
        r2 = subprocess.run([os.path.join(BIN, "hvite"), "-C", str(tmp_path / conf), "-H", str(tmp_path / "MMF"), "-a", "-m", "-L", str(d),
                             "-l", str(d), "-y", "rec", str(tmp_path / "dict"), str(tmp_path / "hmmlist")] + data,
                            capture_output=True, text=True, timeout=900)
        assert r2.returncode == 0, r2.stdout + r2.stderr
        outs[tag] = (lp, (d / "MMF").read_bytes(), [(d / (n + ".rec")).read_text() for n in use])
    assert outs["side"][0] == outs["plain"][0]
    assert outs["side"][1] == outs["plain"][1] and len(outs["side"][1]) > 1000
    assert outs["side"][2] == outs["plain"][2] and all(len(t.split()) >= 15 for t in outs["side"][2])
    r = subprocess.run([os.path.join(BIN, "herest"), "-C", str(tmp_path / "wrong.conf"), "-H", str(tmp_path / "MMF"), "-M", str(tmp_path), "-L", str(tmp_path / "side"),
                        "-m", "1", str(tmp_path / "hmmlist"), os.path.join(GOLD, "data", "spa_1.mfc")], capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "non-matching mask */%%%-*.mfc" in r.stderr, r.stdout + r.stderr


def test_drivers_refuse_what_the_side_files_do_not_fit(native, tmp_path):
    """At load time, with the reference's reasons: a mean file of another kind, a variance file that is not of the target kind, a
    <VARSCALE> vector of another length, a side file that is not there; and _N in the target, whose column the qualifier step has
    dropped before the side vectors are applied (the reference applies them before, HParm.c:2882)."""
    from htk_amd import build as nbuild, synth
    nbuild.build_tools()
    pk = synth.generate(12, 2, 4, 1, 98, 31, D=39).packed()
    names = ["p%d" % i for i in range(pk["numPhys"])]
    synth.write_mmf_packed(str(tmp_path / "MMF"), pk, names, kind="MFCC_E_D_A_Z")
    (tmp_path / "hmmlist").write_text("\n".join(names) + "\n")
    (tmp_path / "spa_1.lab").write_text("p0\np1\n")
    ref = native.cepsnorm_read(os.path.join(GOLD, "cmn", "spa"))
    (tmp_path / "bad").mkdir()
    native.cepsnorm_write(str(tmp_path / "bad" / "spa"), native.parm_kind_parse("MFCC_D_A_0"), "nmv", ref["nFrames"], ref["mean"], ref["var"])
    (tmp_path / "vs38").write_text("<VARSCALE> 38\n" + " 1.0" * 38 + "\n")
    mean = "CMEANDIR = %s/cmn\nCMEANMASK = */%%%%%%_*.mfc\n" % GOLD
    cases = [("TARGETKIND = MFCC_E_D_A_Z\nCMEANDIR = %s\nCMEANMASK = */%%%%%%_*.mfc\n" % (tmp_path / "bad"), "ParmKind mismatch MFCC_D_A_0 not a subset of MFCC_E_D_A_Z"),
             ("TARGETKIND = MFCC_E_D_A_Z\n" + mean + "VARSCALEDIR = %s/cmn\nVARSCALEMASK = */%%%%%%_*.mfc\nVARSCALEFN = %s/varscale\n" % (GOLD, GOLD),
              "ParmKind mismatch MFCC_E_D_A != MFCC_E_D_A_Z"),
             ("TARGETKIND = MFCC_E_D_A_Z\n" + mean + "VARSCALEDIR = %s/cvn\nVARSCALEMASK = */%%%%%%_*.mfc\nVARSCALEFN = %s\n" % (GOLD, tmp_path / "vs38"),
              "mismatch between varScale (38) and target size 39"),
             ("TARGETKIND = MFCC_E_D_A_Z\nCMEANDIR = %s\nCMEANMASK = */%%%%%%_*.mfc\n" % (tmp_path / "nowhere"), "can't open side file"),
             ("TARGETKIND = MFCC_E_D_A_N_Z\n" + mean, "with _N in TARGETKIND is not supported")]
    for conf, why in cases:
        (tmp_path / "c.conf").write_text(conf)
        r = subprocess.run([os.path.join(BIN, "herest"), "-C", str(tmp_path / "c.conf"), "-H", str(tmp_path / "MMF"), "-M", str(tmp_path), "-L", str(tmp_path),
                            "-m", "1", str(tmp_path / "hmmlist"), os.path.join(GOLD, "data", "spa_1.mfc")], capture_output=True, text=True, timeout=900)
        assert r.returncode != 0 and why in r.stderr, (why, r.stdout + r.stderr)


# configuration variable -> frontend_config keyword (value parser), for tests/golden/wave/frontend_a.conf
_VARS = {"SOURCERATE": ("sampPeriod", float), "WINDOWSIZE": ("winDur", float), "TARGETRATE": ("frPeriod", float), "NUMCHANS": ("numChans", int),
         "NUMCEPS": ("numCeps", int), "CEPLIFTER": ("cepLifter", int), "PREEMCOEF": ("preEmph", float), "USEHAMMING": ("useHam", "bool"),
         "USEPOWER": ("usePower", "bool"), "ENORMALISE": ("eNormalise", "bool"), "LPCORDER": ("lpcOrder", int)}


def test_drivers_apply_the_side_mean_to_waveform_sources(native, tmp_path):
    """SOURCEFORMAT = WAV with CMEANDIR / CMEANMASK and TARGETKIND = PLP_0_D_A_Z: the waveform is coded on the device, the qualifiers follow
    without the utterance's own mean, and the side's mean is subtracted -- the same log probability, models and labels as from the
    parameter file of the same statics (the path pinned against HCopy above), and not what plain _Z gives."""
    from htk_amd import build as nbuild, synth
    nbuild.build_tools()
    wgold = os.path.join(ROOT, "tests", "golden", "wave")
    wavconf = open(os.path.join(wgold, "frontend_a.conf")).read()
    kw = {"usePower": False, "eNormalise": True, "numChans": 20}
    for line in wavconf.splitlines():
        k, v = (x.strip() for x in line.split("="))
        if k in _VARS:
            kw[_VARS[k][0]] = (v[0] in "Tt") if _VARS[k][1] == "bool" else _VARS[k][1](v)
    x, _ = native.wave_read(os.path.join(wgold, "test.wav"))
    fe = native.FrontEnd(native.frontend_config("PLP_0", **kw))
    stat, _ = fe.compute_host([x])
    fe.close()
    assert stat.shape[1] == 13
    (tmp_path / "parm").mkdir(); (tmp_path / "cmn").mkdir()
    native.parm_write(str(tmp_path / "parm" / "test.plp"), stat, 100000, native.parm_kind_parse("PLP_0"))
    sideMean = stat.astype(np.float64).mean(0).astype(np.float32) + np.float32(0.5)          # not the utterance's own mean
    native.cepsnorm_write(str(tmp_path / "cmn" / "test"), native.parm_kind_parse("PLP_0"), "m", 0, sideMean, None)
    pk = synth.generate(12, 2, 4, 1, 98, 31, D=39).packed()
    names = ["p%d" % i for i in range(pk["numPhys"])]
    synth.write_mmf_packed(str(tmp_path / "MMF"), pk, names, kind="PLP_0_D_A_Z")
    (tmp_path / "hmmlist").write_text("\n".join(names) + "\n")
    (tmp_path / "dict").write_text("".join("%s %s\n" % (n, n) for n in names))
    side = "CMEANDIR = %s\nCMEANMASK = */%%%%%%%%.*\n" % (tmp_path / "cmn")
    (tmp_path / "wav.conf").write_text(wavconf.replace("PLP_0_D_A", "PLP_0_D_A_Z") + side)
    (tmp_path / "parm.conf").write_text("TARGETKIND = PLP_0_D_A_Z\n" + side)
    (tmp_path / "z.conf").write_text(wavconf.replace("PLP_0_D_A", "PLP_0_D_A_Z"))
    outs = {}
    for tag, conf, data in (("wav", "wav.conf", os.path.join(wgold, "test.wav")), ("parm", "parm.conf", str(tmp_path / "parm" / "test.plp")),
                            ("z", "z.conf", os.path.join(wgold, "test.wav"))):
        d = tmp_path / ("run_" + tag); d.mkdir()
        (d / "test.lab").write_text("\n".join(["p0", "p1", "p2", "p3", "p1"]) + "\n")
        r = subprocess.run([os.path.join(BIN, "herest"), "-C", str(tmp_path / conf), "-H", str(tmp_path / "MMF"), "-M", str(d), "-L", str(d),
                            "-m", "1", "-v", "0.01", str(tmp_path / "hmmlist"), data], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        lp = re.search(r"average log prob per frame = (\S+)", r.stdout).group(1)
        r2 = subprocess.run([os.path.join(BIN, "hvite"), "-C", str(tmp_path / conf), "-H", str(tmp_path / "MMF"), "-a", "-m", "-L", str(d),
                             "-l", str(d), "-y", "rec", str(tmp_path / "dict"), str(tmp_path / "hmmlist"), data], capture_output=True, text=True, timeout=900)
        assert r2.returncode == 0, r2.stdout + r2.stderr
        outs[tag] = (lp, (d / "MMF").read_bytes(), (d / "test.rec").read_text())
    assert outs["wav"] == outs["parm"]
    assert outs["wav"][0] != outs["z"][0] and outs["wav"][1] != outs["z"][1]
