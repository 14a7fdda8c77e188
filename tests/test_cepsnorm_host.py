"""Side-based cepstral mean and variance normalisation, the host part (htk_amd/host/cepsnorm.c): masks, <CEPSNORM> / <VARSCALE> files,
kind and length checks, the scale table.  The fixtures are the reference's (tests/golden/cmvn, make_cmvn_golden.py); no device is needed
and none is looked for before a refusal."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "cmvn")
MASK = "*/%%%_*.mfc"
SIDES = {"spa": 3, "spb": 2, "tpc": 1}
DEVICE_ERR = "no HIP device"


def fixture_files():
    return [os.path.join(GOLD, l.strip()) for l in open(os.path.join(GOLD, "files.lst")) if l.strip()]


def test_mask_matches_the_fixture_names(native):
    got = {}
    for f in fixture_files():
        side = native.mask_match(MASK, f)
        assert side == os.path.basename(f)[:3]
        got[side] = got.get(side, 0) + 1
        assert native.mask_match("*/%??_*.mfc", f) == side[0]
    assert got == SIDES


@pytest.mark.parametrize("mask,name,want", [
    ("*.mfc", "dir/spa_1.mfc", ""),                    # no % in the mask: a match that captures nothing
    ("*%%_*", "a/b/xy_3.mfc", "xy"),                   # * at both ends
    ("*/?%%_*.mfc", "d/spa_1.mfc", "pa"),              # ? takes a character without capturing it
    ("%%%%", "abc", None),                             # a name shorter than the mask
    ("%%%", "abc", "abc"),
    ("*/%%%_*.mfc", "d/spa-1.mfc", None),              # a non-match: no underscore
    ("*/%%%_*.mfc", "spa_1.mfc", None),                # a non-match: no directory
    ("%*%", "abcd", "ad"),                             # the run in the middle is the *'s
    ("*", "", ""),
])
def test_mask_corner_cases(native, mask, name, want):
    assert native.mask_match(mask, name) == want


def test_mask_matcher_against_a_backtracking_regex(native):
    """Every mask over a small alphabet as a regular expression -- * greedy, % a group, ? a dot: the leftmost * takes the longest run that
    leaves a match, which is the reference's preference -- on random names, long runs of * included (the matcher is O(mask x name))."""
    import re
    rng = np.random.default_rng(3)
    for _ in range(3000):
        mask = "".join(rng.choice(list("ab_*%?*%"), rng.integers(0, 8)))
        name = "".join(rng.choice(list("ab_"), rng.integers(0, 9)))
        m = re.fullmatch("".join(".*" if c == "*" else "(.)" if c == "%" else "." if c == "?" else re.escape(c) for c in mask), name, re.S)
        assert native.mask_match(mask, name) == (None if m is None else "".join(m.groups())), (mask, name)
    assert native.mask_match("*a" * 30 + "%", "a" * 200 + "b") == "b" and native.mask_match("*a" * 30 + "%b", "a" * 200) is None


def test_mask_that_captures_more_than_the_buffer_is_refused(native):
    out = C.create_string_buffer(4)
    assert native.lib().htkamd_mask_match(b"%%%%*", b"abcdef", out, 4) == -1
    assert b"captures 4" in native.lib().htkamd_last_error()
    assert native.lib().htkamd_mask_match(b"%%%*", b"abcdef", out, 4) == 1 and out.value == b"abc"


def test_kind_names_round_trip(native):
    for k in ("MFCC_E_D_A", "MFCC_E_D_A_Z", "PLP_D_A_T_0", "FBANK_E_D_N", "MFCC_D_A_Z_0"):
        assert native.parm_kind_str(native.parm_kind_parse(k)) == k
    assert native.parm_kind_parse("MFCC_E_D_A") == 6 | 0o100 | 0o400 | 0o1000
    assert native.parm_kind_parse("MFCC_Q") == -1 and native.parm_kind_parse("NOTAKIND_E") == -1


def test_reading_the_reference_side_files(native):
    nf = {}
    for f in fixture_files():
        x, _, _ = native.parm_read(f)
        nf[os.path.basename(f)[:3]] = nf.get(os.path.basename(f)[:3], 0) + x.shape[0]
    for side in SIDES:
        r = native.cepsnorm_read(os.path.join(GOLD, "cmn", side))
        assert native.parm_kind_str(r["kind"]) == "MFCC_E_D_A" and r["nFrames"] == nf[side]
        assert r["mean"].shape == (39,) and r["var"].shape == (39,) and (r["var"] > 0).all()
        z = native.cepsnorm_read(os.path.join(GOLD, "cvn", side))
        assert native.parm_kind_str(z["kind"]) == "MFCC_E_D_A_Z" and z["nFrames"] == nf[side] and z["mean"] is None and z["var"].shape == (39,)
        p = native.cepsnorm_read(os.path.join(GOLD, "cmn_p", side[0], side))
        assert np.array_equal(p["mean"], r["mean"]) and np.array_equal(p["var"], r["var"])
    # the values are the text's: " %e" read back as strtof reads it
    tok = open(os.path.join(GOLD, "cmn", "spa")).read().split()
    assert np.array_equal(native.cepsnorm_read(os.path.join(GOLD, "cmn", "spa"))["mean"], np.array(tok[6:45], np.float32))


@pytest.mark.parametrize("flags", ["m", "v", "mv", "nv", "nmv"])
def test_writer_reproduces_the_reference_files(native, tmp_path, flags):
    """nmv and nv are files HCompV wrote (cmn/, cvn/); m, v and mv are the nmv file without the lines ExportNMV leaves out."""
    for side in SIDES:
        src = os.path.join(GOLD, "cvn" if flags == "nv" else "cmn", side)
        r = native.cepsnorm_read(src)
        out = str(tmp_path / (side + flags))
        native.cepsnorm_write(out, r["kind"], flags, r["nFrames"], r["mean"], r["var"])
        lines = open(src, "rb").read().split(b"\n")                    # header, <NFRAMES>, [<MEAN> n, values,] <VARIANCE> n, values, ""
        if flags in ("nmv", "nv"):
            want = b"\n".join(lines)
        else:
            assert len(lines) == 7
            keep = [lines[0]] + (lines[2:4] if "m" in flags else []) + (lines[4:6] if "v" in flags else []) + [b""]
            want = b"\n".join(keep)
        assert open(out, "rb").read() == want


def test_writer_refuses_other_flag_sets(native, tmp_path):
    for flags in ("n", "nm", "vm", "x", ""):
        with pytest.raises(native.HtkAmdError) as e:
            native.cepsnorm_write(str(tmp_path / "f"), 6, flags, 1, np.ones(3), np.ones(3))
        assert e.value.rc == -1 and "output flag" in str(e.value)
    with pytest.raises(native.HtkAmdError) as e:
        native.cepsnorm_write(str(tmp_path / "f"), 6, "mv", 1, np.ones(3), None)
    assert "without the vector" in str(e.value)
    assert not os.path.exists(tmp_path / "f")


def test_varscale_file(native, tmp_path):
    v = native.varscale_read(os.path.join(GOLD, "varscale"))
    tok = open(os.path.join(GOLD, "varscale")).read().split()
    assert tok[0] == "<VARSCALE>" and int(tok[1]) == 39 and np.array_equal(v, np.array(tok[2:], np.float32))
    (tmp_path / "bad").write_text("<VARIANCE> 2\n 1.0 2.0\n")
    with pytest.raises(native.HtkAmdError) as e:
        native.varscale_read(str(tmp_path / "bad"))
    assert e.value.rc == -1 and "<VARSCALE> missing" in str(e.value)
    (tmp_path / "short").write_text("<VARSCALE> 3\n 1.0 2.0\n")
    with pytest.raises(native.HtkAmdError) as e:
        native.varscale_read(str(tmp_path / "short"))
    assert "couldn't read" in str(e.value)
    with pytest.raises(native.HtkAmdError) as e:
        native.varscale_read(str(tmp_path / "none"))
    assert e.value.rc == -6 and "can't open" in str(e.value)


def test_side_file_refusals(native, tmp_path):
    (tmp_path / "a").write_text("<MEAN> 2\n 1.0 2.0\n")
    with pytest.raises(native.HtkAmdError) as e:
        native.cepsnorm_read(str(tmp_path / "a"))
    assert e.value.rc == -1 and "<CEPSNORM> missing" in str(e.value)
    (tmp_path / "b").write_text("<CEPSNORM> <MFCC_Q>\n<MEAN> 2\n 1.0 2.0\n")
    with pytest.raises(native.HtkAmdError) as e:
        native.cepsnorm_read(str(tmp_path / "b"))
    assert "unknown parameter kind" in str(e.value)
    (tmp_path / "c").write_text("<CEPSNORM> <MFCC_E>\n<MEAN> 3\n 1.0 2.0\n")
    with pytest.raises(native.HtkAmdError) as e:
        native.cepsnorm_read(str(tmp_path / "c"))
    assert "couldn't read" in str(e.value)
    (tmp_path / "d").write_text("<CEPSNORM> <MFCC_E>\n<VARIANCE> 2\n 1.0 2.0\n")          # <NFRAMES> and <MEAN> are optional
    r = native.cepsnorm_read(str(tmp_path / "d"))
    assert r["nFrames"] is None and r["mean"] is None and list(r["var"]) == [1.0, 2.0]
    with pytest.raises(native.HtkAmdError) as e:
        native.cepsnorm_read(str(tmp_path / "none"))
    assert e.value.rc == -6


def test_kind_checks(native):
    k = native.parm_kind_parse
    native.cepsnorm_check_kinds(k("MFCC_E_D_A_Z"), k("MFCC_E_D_A"), k("MFCC_E_D_A_Z"))
    native.cepsnorm_check_kinds(k("MFCC_E_D_A_Z"), k("MFCC_E"), -1)                       # _D _A _Z of the target are masked for a mean
    native.cepsnorm_check_kinds(k("MFCC_E_D_A_V"), -1, k("MFCC_E_D_A"))                   # a variance may lack only the target's _V
    for mean in ("MFCC_D_A_0", "MFCC_D_A", "PLP_E_D_A", "MFCC_E_D_A_T"):                  # (_T is not in the target: not masked)
        with pytest.raises(native.HtkAmdError) as e:
            native.cepsnorm_check_kinds(k("MFCC_E_D_A_Z"), k(mean), -1)
        assert e.value.rc == -1 and "ParmKind mismatch %s not a subset of MFCC_E_D_A_Z" % mean in str(e.value)
    for var in ("MFCC_E_D_A", "MFCC_E_D_Z", "MFCC_E"):
        with pytest.raises(native.HtkAmdError) as e:
            native.cepsnorm_check_kinds(k("MFCC_E_D_A_Z"), -1, k(var))
        assert e.value.rc == -1 and "ParmKind mismatch %s != MFCC_E_D_A_Z" % var in str(e.value)


def test_scale_table_is_the_reference_expression(native):
    vs = native.varscale_read(os.path.join(GOLD, "varscale"))
    sv = np.stack([native.cepsnorm_read(os.path.join(GOLD, "cmn", s))["var"] for s in SIDES])
    got = native.cepsnorm_scale(vs, sv, list(SIDES))
    assert got.dtype == np.float32 and got.shape == (3, 39)
    assert np.array_equal(got, np.sqrt((vs / sv).astype(np.float32).astype(np.float64)).astype(np.float32))
    rng = np.random.default_rng(5)
    vs = rng.uniform(1e-3, 50, 120).astype(np.float32); sv = rng.uniform(1e-3, 50, (7, 120)).astype(np.float32)
    assert np.array_equal(native.cepsnorm_scale(vs, sv), np.sqrt((vs / sv).astype(np.float32).astype(np.float64)).astype(np.float32))


def test_scale_table_refusals(native):
    vs = np.ones(39, np.float32); sv = np.ones((3, 39), np.float32)
    with pytest.raises(native.HtkAmdError) as e:
        native.cepsnorm_scale(vs[:38], sv, list(SIDES))
    assert e.value.rc == -1 and "mismatch between varScale (38) and target size 39" in str(e.value)
    for bad in (0.0, -1.0, np.nan):
        sv2 = sv.copy(); sv2[1, 4] = bad
        with pytest.raises(native.HtkAmdError) as e:
            native.cepsnorm_scale(vs, sv2, list(SIDES))
        assert e.value.rc == -1 and "side spb" in str(e.value) and "not positive" in str(e.value)
        with pytest.raises(native.HtkAmdError) as e:
            native.cepsnorm_scale(vs, sv2)
        assert "side 1" in str(e.value)


def test_finishing_the_statistics(native):
    rng = np.random.default_rng(9)
    x = [rng.normal(3.0, 2.0, (n, 5)) for n in (40, 1, 0)]
    s = np.stack([a.sum(0) for a in x]); q = np.stack([(a * a).sum(0) for a in x]); n = np.array([40, 1, 0])
    mean, var = native.side_stats_finish(s, q, n)
    m = s[:2] / n[:2, None]
    assert np.array_equal(mean[:2], m.astype(np.float32)) and np.array_equal(var[:2], (q[:2] / n[:2, None] - m * m).astype(np.float32))
    assert not mean[2].any() and not var[2].any()                      # a side without frames keeps zeros


def test_symbols_are_exported(native):
    L = native.lib()
    for name in ("htkamd_mask_match", "htkamd_cepsnorm_read", "htkamd_cepsnorm_write", "htkamd_varscale_read", "htkamd_cepsnorm_check_kinds",
                 "htkamd_cepsnorm_scale", "htkamd_side_stats", "htkamd_side_stats_finish", "htkamd_parm_normalise", "htkamd_parm_kind_parse",
                 "htkamd_parm_kind_str"):
        assert hasattr(L, name), name


def test_device_entry_points_check_arguments_first_and_then_want_a_device(native):
    """Bad arguments are HTKAMD_EINVAL whether a device is there or not; good ones are HTKAMD_ENODEV without one."""
    off = np.array([0, 3, 5], np.int32)
    for side in ([0, 2], [-1, 0]):
        with pytest.raises(native.HtkAmdError) as e:
            native.side_stats(C.c_void_p(16), off, side, 2, 39, 39)
        assert e.value.rc == -1 and "side %d of 2" % side[0 if side[0] < 0 else 1] in str(e.value) and DEVICE_ERR not in str(e.value)
        with pytest.raises(native.HtkAmdError) as e:
            native.parm_normalise(C.c_void_p(16), off, side, 2, 39, mean=np.zeros((2, 13), np.float32))
        assert e.value.rc == -1 and DEVICE_ERR not in str(e.value)
    with pytest.raises(native.HtkAmdError) as e:
        native.side_stats(C.c_void_p(16), off, [0, 1], 2, 13, 39)                        # D beyond the row
    assert e.value.rc == -1
    with pytest.raises(native.HtkAmdError) as e:
        native.parm_normalise(C.c_void_p(16), off, [0, 1], 2, 13, mean=np.zeros((2, 39), np.float32))
    assert e.value.rc == -1 and "39 mean" in str(e.value)
    with pytest.raises(native.HtkAmdError) as e:
        native.parm_normalise(C.c_void_p(16), np.array([0, 5, 3], np.int32), [0, 1], 2, 39, mean=np.zeros((2, 39), np.float32))
    assert e.value.rc == -1 and "monotone" in str(e.value)
    if native.lib().htkamd_device_count() == 0:
        with pytest.raises(native.HtkAmdError) as e:
            native.side_stats(C.c_void_p(16), off, [0, 1], 2, 39, 39)
        assert e.value.rc == -2 and DEVICE_ERR in str(e.value)
        with pytest.raises(native.HtkAmdError) as e:
            native.parm_normalise(C.c_void_p(16), off, [0, 1], 2, 39, mean=np.zeros((2, 39), np.float32))
        assert e.value.rc == -2 and DEVICE_ERR in str(e.value)


def run_tool(tool, conf_text, tmp_path, data):
    import subprocess
    (tmp_path / "c.conf").write_text(conf_text.replace("@GOLD@", GOLD))
    (tmp_path / "hmmlist").write_text("p0\n")
    return subprocess.run([os.path.join(ROOT, "tools", "bin", tool), "-C", str(tmp_path / "c.conf")] + (["-a", "dict"] if tool == "hvite" else []) +
                          [str(tmp_path / "hmmlist"), data], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("tool", ["herest", "hvite"])
def test_drivers_refuse_an_incomplete_configuration_before_a_device(native, tmp_path, tool):
    from htk_amd import build as nbuild
    nbuild.build_tools()
    data = fixture_files()[0]
    for conf, why in (("CMEANDIR = @GOLD@/cmn\n", "mask or dir missing"), ("CMEANMASK = */%%%_*.mfc\n", "mask or dir missing"),
                      ("VARSCALEDIR = @GOLD@/cmn\nVARSCALEFN = @GOLD@/varscale\n", "mask or dir missing"),
                      ("VARSCALEDIR = @GOLD@/cmn\nVARSCALEMASK = */%%%_*.mfc\n", "without VARSCALEFN"),
                      ("VARSCALEFN = @GOLD@/varscale\n", "no variance scaling vector found"),
                      ("CMEANDIR = @GOLD@/cmn\nCMEANMASK = */%%%_*.mfc\nMATTRANFN = x\n", "MATTRANFN")):
        r = run_tool(tool, "TARGETKIND = MFCC_E_D_A_Z\n" + conf, tmp_path, data)
        assert r.returncode != 0 and why in r.stderr and DEVICE_ERR not in r.stderr, r.stderr
    # without side normalisation the variables of the steps this path does not serve are none of its business, as before
    r = run_tool(tool, "TARGETKIND = MFCC_E_D_A_Z\nMATTRANFN = x\nHIGHDIFF = T\n", tmp_path, data)
    assert "MATTRANFN" not in r.stderr and "HIGHDIFF" not in r.stderr, r.stderr
    r = subprocess_help(tool)
    for v in ("CMEANDIR", "CMEANMASK", "CMEANPATHMASK", "VARSCALEDIR", "VARSCALEMASK", "VARSCALEPATHMASK", "VARSCALEFN"):
        assert v in r


def subprocess_help(tool):
    import subprocess
    r = subprocess.run([os.path.join(ROOT, "tools", "bin", tool), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    return r.stdout
