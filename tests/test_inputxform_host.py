"""Global linear input transforms on the host (htk_amd/host/mmf.c): <INPUTXFORM> of a model set inline and as ~j "name", ~j macros,
transform files of their own, the writer against the reference's HHEd, the checks of a transform against the data and the set it meets,
and the drivers' refusals -- all against tests/golden/inputxform (make_inputxform_golden.py).  No device is needed here."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inputxform_util import macro_form, read_xform_text  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "inputxform")
SETS = os.path.join(GOLD, "sets")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")
LIST = os.path.join(SETS, "hmmlist")
DEVICE_ERR = "no HIP device"


def load(native, name):
    return native.Mmf(files=[os.path.join(SETS, name)], hmm_list=LIST)


def macro_set(tmp_path):
    """the ~j form of the set: the macro's definition, then the set that names it, in one file"""
    (tmp_path / "macro.mmf").write_text("".join(macro_form(open(os.path.join(SETS, "inline.mmf")).read())))
    return str(tmp_path / "macro.mmf")


def fileref_set(tmp_path, name="proj20"):
    """the ~j form's two halves as two files: the macro as a transform file, and beside it the set that names it"""
    macro, rest = macro_form(open(os.path.join(SETS, "inline.mmf")).read())
    (tmp_path / "proj20").write_text(macro)
    (tmp_path / "fileref.mmf").write_text(rest.replace('~j "proj20"', '~j "%s"' % name))
    return str(tmp_path / "fileref.mmf")


def write_back(native, mmf, path, binary):
    import ctypes as C
    pk = mmf.packed()
    g = np.zeros(len(pk["var"]), np.float32)          # the reference computes every gConst anew at load (FixAllGConsts) and writes those
    for i in range(len(g)):
        native.lib().htkamd_host_fix_diag_gconst(C.c_int(pk["var"].shape[1]), np.ascontiguousarray(pk["var"][i]).ctypes.data_as(C.c_void_p),
                                                 g[i:i + 1].ctypes.data_as(C.c_void_p))
    mmf.write(dict(mean=pk["mean"], var=pk["var"], gconst=g, compWeight=pk["compWeight"], transP=pk["transP"]), one_file=str(path), binary=binary)
    return open(path, "rb").read()


def extra_macro_set(tmp_path):
    """the ~j form with a second ~j macro that nobody names"""
    macro, rest = macro_form(open(os.path.join(SETS, "inline.mmf")).read())
    (tmp_path / "extra.mmf").write_text(macro + macro.replace('"proj20"', '"unused"') + rest)
    return str(tmp_path / "extra.mmf")


MADE = {"macro.mmf": macro_set, "fileref.mmf": fileref_set, "extra.mmf": extra_macro_set}


@pytest.mark.parametrize("name", ["inline.mmf", "macro.mmf", "fileref.mmf", "extra.mmf", "inline_bin.mmf", "macro_bin.mmf"])
def test_transformed_sets_load_and_are_written_back_as_the_reference_writes_them(native, tmp_path, name):
    """Both forms, text and binary: the accessors give the fixture's transform, and the set written back unchanged is HHEd's re-save
    byte for byte -- inline.mmf and inline_bin.mmf, for either form: a transform read either way is written in full behind the global
    options, and a ~j macro nobody names is not written at all (PutOptions HModel.c:3257, SaveMacros :4350; the generator checked HHEd's
    re-saves of the ~j form, text and binary, and of the set with an unused ~j macro against these two files)."""
    want = read_xform_text(os.path.join(GOLD, "xf", "proj20"))              # the matrix the generator put into the sets
    path = MADE[name](tmp_path) if name in MADE else os.path.join(SETS, name)
    mmf = native.Mmf(files=[path], hmm_list=LIST)
    xf = mmf.input_xform
    assert xf is not None and mmf.set_id == "demo20" and mmf.kind == "MFCC_E_D_A" and mmf.desc.vecSize == 20
    assert (xf.mask, xf.kind, xf.prequal, xf.rows, xf.cols, xf.vec_size) == ("demo*", "MFCC_E_D_A", False, 20, 39, 20)
    assert xf.matrix.tobytes() == want["matrix"].tobytes() and xf.bias is None and xf.logdet == 0.0
    assert xf.name == (path if name.startswith("inline") else "proj20")               # inline: known by its file (HModel.c:650)
    assert write_back(native, mmf, tmp_path / "t.mmf", False) == open(os.path.join(SETS, "inline.mmf"), "rb").read()
    assert write_back(native, mmf, tmp_path / "b.mmf", True) == open(os.path.join(SETS, "inline_bin.mmf"), "rb").read()


def test_a_set_without_a_transform_has_none(native):
    mmf = native.Mmf(files=[os.path.join(ROOT, "tests", "golden", "mmf", "syn_in.mmf")], hmm_list=os.path.join(ROOT, "tests", "golden", "mmf", "syn_list"))
    assert mmf.input_xform is None and mmf.set_id == ""


@pytest.mark.parametrize("name,shape,kind,prequal", [("full39", (39, 39), "MFCC_E_D_A", False), ("proj20", (20, 39), "MFCC_E_D_A", False),
                                                     ("pre13", (13, 13), "MFCC_E", True), ("exp45", (45, 39), "MFCC_E_D_A", False)])
def test_transform_files_round_trip(native, tmp_path, name, shape, kind, prequal):
    src = os.path.join(GOLD, "xf", name)
    x = native.InputXForm.read(src)
    binary = name in ("full39", "exp45")                                            # the fixture's two large files are binary ones
    assert (x.name, x.mask, x.kind, x.prequal, x.matrix.shape) == (name, "*", kind, prequal, shape)
    x.write(str(tmp_path / "t"), binary=binary)
    assert open(tmp_path / "t", "rb").read() == open(src, "rb").read()              # the generator wrote it as SaveInputXForm does
    if not binary:
        assert x.matrix.tobytes() == read_xform_text(src)["matrix"].tobytes()
    x.write(str(tmp_path / "b"), binary=not binary)
    y = native.InputXForm.read(str(tmp_path / "b"))
    assert (y.name, y.mask, y.kind, y.prequal) == (x.name, x.mask, x.kind, x.prequal) and y.matrix.tobytes() == x.matrix.tobytes()


def test_bias_and_logdet_are_carried_in_text_and_binary(native, tmp_path):
    x = native.InputXForm.read(os.path.join(GOLD, "xf", "pre13b"))
    b = native.InputXForm.read(os.path.join(GOLD, "xf", "pre13b.bin"))
    for t in (x, b):
        assert t.name == "pre13b" and t.mask == "demo*" and t.prequal and t.bias is not None and t.bias.shape == (13,) and t.logdet == -3.25
    assert x.bias.tobytes() == b.bias.tobytes() and x.matrix.tobytes() == b.matrix.tobytes()
    x.write(str(tmp_path / "t")); b.write(str(tmp_path / "b"), binary=True)
    assert open(tmp_path / "t", "rb").read() == open(os.path.join(GOLD, "xf", "pre13b"), "rb").read()
    assert open(tmp_path / "b", "rb").read() == open(os.path.join(GOLD, "xf", "pre13b.bin"), "rb").read()
    # without its ~j header a transform file is known by the file's name (LoadInputXForm HModel.c:4660)
    body = open(os.path.join(GOLD, "xf", "pre13b")).read().split("\n", 1)[1]
    (tmp_path / "bare").write_text(body)
    assert native.InputXForm.read(str(tmp_path / "bare")).name == str(tmp_path / "bare")


def edited(tmp_path, name, old, new):
    text = open(os.path.join(SETS, "inline.mmf")).read()
    assert old in text
    (tmp_path / name).write_text(text.replace(old, new, 1))
    return str(tmp_path / name)


def test_refusals_of_the_reader(native, tmp_path):
    with pytest.raises(native.HtkAmdError) as e:      # two blocks (SetInputXFormConfig HParm.c:631)
        native.Mmf(files=[edited(tmp_path, "two.mmf", "<BLOCKINFO> 1 20", "<BLOCKINFO> 2 10 10")], hmm_list=LIST)
    assert "only full linear transforms are supported" in str(e.value)
    with pytest.raises(native.HtkAmdError) as e:      # a ~j name that is neither a macro nor a file
        native.Mmf(files=[fileref_set(tmp_path, "nowhere")], hmm_list=LIST)
    assert 'undefined ~j macro "nowhere", and no file of that name' in str(e.value)
    for old, new, why in (("<INPUTXFORM><MMFIDMASK>", "<INPUTXFORM><LINXFORM>", "<MMFIDMASK> symbol expected"),
                          ("<XFORM> 20 39", "<XFORM> 20 40", "number expected"),
                          ("<INPUTXFORM>", "<PARENTXFORM> ~a \"x\"\n<INPUTXFORM>", "unsupported global option")):
        with pytest.raises(native.HtkAmdError) as e:
            native.Mmf(files=[edited(tmp_path, "bad.mmf", old, new)], hmm_list=LIST)
        assert why in str(e.value), (why, str(e.value))
    for macro in ("a", "b", "g", "f"):                # the other transform macros stay refused
        (tmp_path / "m.mmf").write_text('~%s "x"\n<ADAPTKIND> BASE\n' % macro)
        with pytest.raises(native.HtkAmdError) as e:
            native.Mmf(files=[str(tmp_path / "m.mmf")])
        assert "unsupported macro type" in str(e.value)


def test_checks_of_a_transform_against_data_and_set(native):
    """htkamd_inputxform_check: each of the reference's checks with its own message."""
    xf = load(native, "inline.mmf").input_xform
    xf.check_against("MFCC_E", "MFCC_E_D_A", 13, "demo20", 20)
    cases = [(("MFCC_0", "MFCC_0_D_A", 13, "demo20", 20), "does not fit the data's MFCC_0"),                  # HParm.c:1636-1642
             (("PLP_E", "PLP_E_D_A", 13, "demo20", 20), "does not fit the data's PLP_E"),
             (("MFCC_E", "MFCC_E_D_A_Z", 13, "demo20", 20), "is not the qualified data's MFCC_E_D_A_Z"),       # HParm.c:1835
             (("MFCC_E", "MFCC_E_D", 13, "demo20", 20), "is not the qualified data's MFCC_E_D"),
             (("MFCC_E", "MFCC_E_D_A", 14, "demo20", 20), "39 matrix columns for rows of 42 values"),          # HParm.c:1256
             (("MFCC_E", "MFCC_E_D_A", 13, "demo20", 39), "<VECSIZE> 39 differs from the 20 values the transform produces"),
             (("MFCC_E", "MFCC_E_D_A", 13, "other", 20), "HMM set other is not compatible with <MMFIDMASK> demo*"),   # HParm.c:691
             (("MFCC_E", "MFCC_E_D_A_N", 13, "demo20", 20), "_N")]
    for args, why in cases:
        with pytest.raises(native.HtkAmdError) as e:
            xf.check_against(*args)
        assert why in str(e.value), (args, str(e.value))
    pre = native.InputXForm.read(os.path.join(GOLD, "xf", "pre13"))
    pre.check_against("MFCC_E", "MFCC_E_D_A_Z", 13, "anything", 39)                                            # rows x (1 + deltas present), HParm.c:2203
    for args, why in [(("MFCC_E_Z", "MFCC_E_D_A_Z", 13, "", 39), "disagree in _Z"),                            # HParm.c:1646
                      (("MFCC_E", "MFCC_E_D_A", 12, "", 39), "13 matrix columns for rows of 12 values"),
                      (("MFCC_E", "MFCC_E_D_A", 13, "", 13), "<VECSIZE> 13 differs from the 39 values")]:
        with pytest.raises(native.HtkAmdError) as e:
            pre.check_against(*args)
        assert why in str(e.value), (args, str(e.value))


def test_device_entry_points_fail_loudly_without_a_device(native):
    import ctypes as C
    L = native.lib()
    # argument checks come first, device or not
    assert L.htkamd_parm_xform(None, C.c_int(39), None, C.c_int(39), C.c_longlong(0), None, C.c_int(129), C.c_int(39), None) == -1
    assert b"at most 128 x 128" in L.htkamd_last_error()
    assert L.htkamd_parm_xform(None, C.c_int(13), None, C.c_int(39), C.c_longlong(0), None, C.c_int(20), C.c_int(39), None) == -1
    assert b"39 matrix columns for input rows of 13" in L.htkamd_last_error()
    if L.htkamd_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(native.HtkAmdError) as e:
        native.parm_xform(None, 39, None, 39, 0, None, 20, 39)
    assert "parm_xform: no HIP device" in str(e.value)
    xf = load(native, "inline.mmf").input_xform
    q = native.parm_quals_from_kind("MFCC_E_D_A", 13)
    frameOff = np.array([0, 3], np.int32)
    assert L.htkamd_inputxform_apply(xf.h, None, frameOff.ctypes.data_as(C.c_void_p), C.c_int(1), C.byref(q), None, None) == -2
    assert b"inputxform_apply: no HIP device" in L.htkamd_last_error()


@pytest.mark.parametrize("tool", ["herest", "hvite"])
def test_drivers_refuse_a_transformed_set_with_side_normalisation_before_a_device(native, tmp_path, tool):
    from htk_amd import build as nbuild
    nbuild.build_tools()
    cmvn = os.path.join(ROOT, "tests", "golden", "cmvn")
    data = os.path.join(DEMO, "train", "tr1.mfc")
    for conf in ("CMEANDIR = %s/cmn\nCMEANMASK = */%%%%%%_*.mfc\n" % cmvn, "VARSCALEDIR = %s/cmn\nVARSCALEMASK = */%%%%%%_*.mfc\nVARSCALEFN = %s/varscale\n" % (cmvn, cmvn)):
        (tmp_path / "c.conf").write_text("TARGETKIND = MFCC_E_D_A\n" + conf)
        if tool == "herest":
            cmd = [os.path.join(ROOT, "tools", "bin", "herest"), "-C", str(tmp_path / "c.conf"), "-H", os.path.join(SETS, "inline.mmf"), "-M", str(tmp_path),
                   "-L", os.path.join(DEMO, "labels"), LIST, data]
        else:
            cmd = [os.path.join(ROOT, "tools", "bin", "hvite"), "-C", str(tmp_path / "c.conf"), "-H", os.path.join(SETS, "inline.mmf"), "-a", "-L", os.path.join(DEMO, "labels"),
                   "-l", str(tmp_path), os.path.join(DEMO, "bcpvocab"), LIST, data]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "INPUTXFORM" in r.stderr and DEVICE_ERR not in r.stderr, r.stderr


def test_reader_and_writer_under_sanitizers(native, tmp_path):
    """mmf.c's transform reader and writer under AddressSanitizer + UndefinedBehaviorSanitizer through a stand-alone program with the
    sanitizers' runtimes linked in (tests/inputxform_sanitize.c): every fixture set and transform file, whole and truncated."""
    asan = subprocess.run(["gcc", "-print-file-name=libasan.a"], capture_output=True, text=True).stdout.strip()
    static = ["-static-libasan", "-static-libubsan"] if os.path.isabs(asan) and os.path.exists(asan) else []      # else the shared runtimes: the program links them itself
    exe = str(tmp_path / "inputxform_sanitize")
    host = os.path.join(ROOT, "htk_amd", "host")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined"] + static + ["-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "inputxform_sanitize.c")] +
                          [os.path.join(host, f) for f in ("mmf.c", "prep.c", "cepsnorm.c", "accio.c", "htktext.c")] + ["-lm"])
    files = [os.path.join(SETS, "inline.mmf"), macro_set(tmp_path), extra_macro_set(tmp_path), os.path.join(SETS, "inline_bin.mmf"), os.path.join(SETS, "macro_bin.mmf")] + \
            [os.path.join(GOLD, "xf", f) for f in ("pre13b", "pre13b.bin", "pre13", "exp45")]
    scratch = tmp_path / "scratch"; scratch.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(scratch), LIST] + files, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK %d " % len(files)), (r.stdout[-2000:], r.stderr[-4000:])
