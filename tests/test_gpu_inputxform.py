"""Global linear input transforms on the device (htk_amd/csrc/inputxform.hip): htkamd_parm_xform against the NumPy float32 restatement of
ApplyStaticMat's loop, bit for bit; htkamd_inputxform_apply (transform and qualifiers in the reference's order) against the files the
reference's HCopy wrote under MATTRANFN; and alignment / re-estimation through a 20 x 39 transformed set against the reference's HVite
and HERest (tests/golden/inputxform, make_inputxform_golden.py), through the library and through the command-line drivers."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inputxform_util import macro_form, with_kind, xform_ref  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "inputxform")
SETS = os.path.join(GOLD, "sets")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")
BIN = os.path.join(ROOT, "tools", "bin")
E2E = ["tr1", "tr3"]

MCOLS = [1, 13, 39, 64, 65, 128]          # 16 / 40 / 64 / 128 are the kernel's register forms: 13, 39, 64 and 65, 128 sit at their edges
MROWS = [1, 13, 20, 39, 45, 65, 128]
NROWS = [1, 63, 64, 65, 257]              # a wavefront owns 64 rows


def cases():
    """(mrows, mcols, nRows, inCols, outCols, in place): every listed size at least three times, 33 cases"""
    out = []
    for i, mc in enumerate(MCOLS):
        for j, mr in enumerate(MROWS):
            if (i + j) % 2 == 0:
                out.append((mr, mc, NROWS[(3 * i + j) % 5], mc, mr, False))
    out += [(20, 39, 65, 52, 24, False), (45, 39, 257, 40, 64, False), (13, 13, 63, 39, 39, False), (128, 128, 64, 130, 129, False),     # strides wider than the matrix
            (1, 1, 257, 3, 2, False), (39, 65, 1, 70, 39, False)]
    out += [(39, 39, 257, 39, 39, True), (20, 39, 65, 52, 52, True), (45, 39, 64, 45, 45, True), (13, 13, 63, 39, 39, True),           # in place, equal strides
            (128, 128, 65, 128, 128, True), (1, 64, 1, 64, 64, True)]
    return out


def mixed(rng, shape):
    return (rng.normal(0.0, 1.0, shape) * 10.0 ** rng.uniform(-3, 2, shape)).astype(np.float32)


def run_xform(native, M, X, outCols, inplace, fill):
    """-> (first mrows columns, the other columns of the output table, the input table afterwards)"""
    mrows, mcols = M.shape
    nRows, inCols = X.shape
    dM = native.DevArray(M)
    dIn = native.DevArray(X)
    if inplace:
        assert outCols == inCols
        dOut = dIn
    else:
        dOut = native.DevArray(fill)
    native.parm_xform(dIn.ptr, inCols, dOut.ptr, outCols, nRows, dM.ptr, mrows, mcols)
    native.check(native.lib().htkamd_stream_sync(None), "stream_sync")
    out = dOut.to_host(np.float32, (nRows, outCols))
    return out[:, :mrows], out[:, mrows:], dIn.to_host(np.float32, (nRows, inCols))


@pytest.mark.parametrize("mrows,mcols,nRows,inCols,outCols,inplace", cases())
def test_parm_xform_is_the_restatement_bit_for_bit(native, mrows, mcols, nRows, inCols, outCols, inplace):
    rng = np.random.default_rng(1000 * mrows + mcols + nRows)
    M, X = mixed(rng, (mrows, mcols)), mixed(rng, (nRows, inCols))
    fill = X if inplace else mixed(rng, (nRows, outCols))
    got, rest, after = run_xform(native, M, X, outCols, inplace, fill)
    assert got.tobytes() == xform_ref(M, X[:, :mcols]).tobytes()
    assert rest.tobytes() == fill[:, mrows:].tobytes()                      # columns beyond mrows are left untouched
    if not inplace:
        assert after.tobytes() == X.tobytes()


def test_parm_xform_keeps_subnormal_products_and_sums(native):
    rng = np.random.default_rng(5)
    M = (rng.uniform(0.5, 2.0, (20, 39)) * rng.choice([-1.0, 1.0], (20, 39)) * 1e-20).astype(np.float32)
    X = (rng.uniform(0.5, 2.0, (65, 39)) * rng.choice([-1.0, 1.0], (65, 39)) * 1e-21).astype(np.float32)      # products near 1e-41: subnormal
    want = xform_ref(M, X)
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert (want != 0).all() and (np.abs(want) < tiny).all()                # every sum is subnormal: flushing to zero would give 0.0
    got, _, _ = run_xform(native, M, X, 20, False, np.zeros((65, 20), np.float32))
    assert got.tobytes() == want.tobytes()


def test_parm_xform_with_negative_zero_inputs(native):
    rng = np.random.default_rng(6)
    M = mixed(rng, (13, 13)); M[3] = 0.0; M[5] = -np.abs(M[5])
    X = mixed(rng, (64, 13)); X[7] = -0.0; X[9, ::2] = -0.0; X[11] = 0.0
    want = xform_ref(M, X)
    got, _, _ = run_xform(native, M, X, 13, False, np.ones((64, 13), np.float32))
    assert got.tobytes() == want.tobytes()                                  # bits, the sign of zero among them
    assert not np.signbit(want[7]).any()                                    # 0.0f + (m * -0.0f) is +0.0f, as in the reference


def xform_file(tmp_path, name, target):
    """xf/<name>; applied after the qualifiers a transform must carry the kind of the qualified rows (HParm.c:1835), so for a _Z target
    the committed file is rewritten with that kind, as the fixture's generator did for HCopy"""
    src = os.path.join(GOLD, "xf", name)
    if name == "pre13" or not target.endswith("_Z"):
        return src
    return with_kind(src, str(tmp_path / name))


@pytest.mark.parametrize("name", ["full39", "proj20", "pre13", "exp45"])
@pytest.mark.parametrize("target", ["MFCC_E_D_A", "MFCC_E_D_A_Z"])
def test_qualifiers_and_transform_in_the_documented_order_equal_hcopy(native, tmp_path, name, target):
    """htkamd_inputxform_apply on the fixture's statics == the files HCopy wrote under MATTRANFN, every value bit for bit: after the
    qualifiers (39 x 39, the 20 x 39 projection, the 45 x 39 expansion) and <PREQUAL> (13 x 13, where _Z takes the mean off every static)."""
    xf = native.InputXForm.read(xform_file(tmp_path, name, target))
    stat = [native.parm_read(os.path.join(GOLD, "data", f + ".mfc"))[0] for f in "abc"]
    assert [x.shape for x in stat] == [(9, 13), (33, 13), (1, 13)]
    xf.check_against("MFCC_E", target, 13)
    dX, frameOff, cols = xf.apply(stat, native.parm_quals_from_kind(target, 13))
    assert cols == (39 if name == "pre13" else xf.rows)
    got = dX.to_host(np.float32, (int(frameOff[-1]), cols))
    for u, f in enumerate("abc"):
        want = native.parm_read(os.path.join(GOLD, "out", name, target, f + ".htk"))[0]
        assert got[frameOff[u]:frameOff[u + 1]].tobytes() == want.tobytes(), (name, target, f)


def demo_batch(native, mmf):
    stat, seqs = [], []
    for u in E2E:
        X, period, kind = native.parm_read(os.path.join(DEMO, "train", u + ".mfc"))
        stat.append(X)
        seqs.append(np.array([mmf.logical[n] for n, _, _, _ in native.labels_read(os.path.join(DEMO, "labels", u + ".lab"))], np.int32))
    xf = mmf.input_xform
    xf.check_against("MFCC_E", "MFCC_E_D_A", 13, mmf.set_id, mmf.desc.vecSize)
    dX, frameOff, cols = xf.apply(stat, native.parm_quals_from_kind("MFCC_E_D_A", 13))
    assert cols == 20 == mmf.desc.vecSize
    labOff = np.concatenate([[0], np.cumsum([len(q) for q in seqs])]).astype(np.int32)
    return dX, frameOff, labOff, seqs


def close_to_reference_set(ours_path):
    """against the set HERest wrote: the options and the transform (everything before the first model: inline.mmf's head, as the
    generator checked of HERest's file) byte for byte, every parameter of e2e/herest.models to the project's 1e-4"""
    ours, head = open(ours_path).read(), open(os.path.join(SETS, "inline.mmf")).read()
    head = head[:head.index("~h ")]
    assert "<INPUTXFORM>" in head and ours[:ours.index("~h ")] == head
    a, b = ours[ours.index("~h "):].split(), open(os.path.join(GOLD, "e2e", "herest.models")).read().split()
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x != y:
            assert abs(float(x) - float(y)) <= 1e-4 * max(abs(float(y)), 1e-3), (x, y)


def test_alignment_and_reestimation_through_the_transformed_set(native, tmp_path):
    mmf = native.Mmf(files=[os.path.join(SETS, "inline.mmf")], hmm_list=os.path.join(SETS, "hmmlist"))
    model = native.Model(mmf.packed())
    dX, frameOff, labOff, seqs = demo_batch(native, mmf)
    # HVite -a -m -f: the label files byte for byte
    res = native.Viterbi(model).align(dX.ptr.value, frameOff, labOff, np.concatenate(seqs))
    for u, r in zip(E2E, res):
        assert r["status"] == 1
        assert "".join(l + "\n" for l in native.format_rec(r, mmf.phys_names)) == open(os.path.join(GOLD, "e2e", "rec", u + ".rec")).read(), u
    # one HERest iteration (-t 2000.0, defaults otherwise)
    fb, acc = native.ForwardBackward(model), native.Accs(model)
    fb.prepare(dX.ptr.value, frameOff, labOff, np.concatenate(seqs))
    fb.execute(native.fb_config(pruneInit=2000.0, pruneInc=0.0, pruneLim=2000.0), acc)
    pr, st = fb.results()
    assert (st == 1).all()
    log = open(os.path.join(GOLD, "e2e", "herest.log")).read()
    T = np.diff(frameOff)
    for u, name in enumerate(E2E):
        assert "%e" % (pr[u] / T[u]) in log.split("Data: %s.mfc" % name)[1].split("\n")[1], name
    a = acc.download()
    model.update(acc, a["vec"])
    mmf.write(model.get_params(), one_file=str(tmp_path / "new.mmf"))
    close_to_reference_set(str(tmp_path / "new.mmf"))


def test_drivers_honour_the_transform_of_the_set_they_load(native, tmp_path):
    from htk_amd import build as nbuild
    nbuild.build_tools()
    (tmp_path / "c.conf").write_text("TARGETKIND = MFCC_E_D_A\n")
    files = [os.path.join(DEMO, "train", u + ".mfc") for u in E2E]
    (tmp_path / "macro.mmf").write_text("".join(macro_form(open(os.path.join(SETS, "inline.mmf")).read())))      # the ~j form of the set
    for form, path in (("inline", os.path.join(SETS, "inline.mmf")), ("macro", str(tmp_path / "macro.mmf"))):
        rec = tmp_path / ("rec_" + form); rec.mkdir()
        r = subprocess.run([os.path.join(BIN, "hvite"), "-C", str(tmp_path / "c.conf"), "-H", path, "-a", "-m", "-f", "-L", os.path.join(DEMO, "labels"),
                            "-l", str(rec), os.path.join(DEMO, "bcpvocab"), os.path.join(SETS, "hmmlist")] + files, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        for u in E2E:
            assert (rec / (u + ".rec")).read_bytes() == open(os.path.join(GOLD, "e2e", "rec", u + ".rec"), "rb").read(), (form, u)
    new = tmp_path / "new"; new.mkdir()
    r = subprocess.run([os.path.join(BIN, "herest"), "-C", str(tmp_path / "c.conf"), "-H", os.path.join(SETS, "inline.mmf"), "-M", str(new), "-L", os.path.join(DEMO, "labels"),
                        "-t", "2000.0", os.path.join(SETS, "hmmlist")] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    close_to_reference_set(str(new / "inline.mmf"))


def test_example_writes_what_hcopy_writes_under_mattranfn(native, tmp_path):
    """examples/input_xform.py as a user runs it: a transform file, parameter files in, parameter files out."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import input_xform
    files = [os.path.join(GOLD, "data", f + ".mfc") for f in "abc"]
    for name, target in (("proj20", "MFCC_E_D_A_Z"), ("pre13", "MFCC_E_D_A")):
        out = input_xform.main(["--xform", xform_file(tmp_path, name, target), "--kind", target, "-d", str(tmp_path / (name + "_out"))] + files)
        for p, f in zip(out, "abc"):
            want = native.parm_read(os.path.join(GOLD, "out", name, target, f + ".htk"))[0]
            assert native.parm_read(p)[0].tobytes() == want.tobytes(), (name, f)


def test_hvite_honours_the_transform_behind_a_waveform_source(native, tmp_path):
    """tools/bin/hvite codes tests/golden/wave/test.wav on the device (MFCC_0 statics), and the set's transform -- <INPUTXFORM> ~j "full39",
    the binary transform file beside the set -- follows the qualifiers as for parameter files: the label file against the reference
    HVite's, which coded the waveform itself (e2e/wav_align.rec).  Names and boundaries are held exactly; the scores to 1e-3 x max(1, |score|),
    the rule tests/test_cli_tools.py holds waveform-coded scores to (the device front end is bit-equal to the reference's in > 99.9 % of
    its values and 1 ulp off in the rest, which seven printed digits of a score of 1e6 can show)."""
    from htk_amd import build as nbuild
    nbuild.build_tools()
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_wav_labels_golden as g
    from inputxform_util import wav_case_set
    wave = os.path.join(ROOT, "tests", "golden", "wave")
    d = str(tmp_path)
    (tmp_path / "xf.mmf").write_text(wav_case_set(open(os.path.join(wave, "fitted.mmf")).read(), ' ~j "full39"\n'))
    with_kind(os.path.join(GOLD, "xf", "full39"), str(tmp_path / "full39"), new="<MFCC_0_D_A>")
    g.write_case(d, "WAV", mmf=str(tmp_path / "xf.mmf"))
    ours = g.run_tool(os.path.join(BIN, "hvite"), d, os.path.join(wave, "test.wav"), "align")
    want = open(os.path.join(GOLD, "e2e", "wav_align.rec")).read().splitlines()
    assert len(ours) == len(want)
    for a, b in zip(ours, want):
        a, b = a.split(), b.split()
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            if i in (3, 5):
                assert abs(float(x) - float(y)) <= 1e-3 * max(1.0, abs(float(y))), (a, b)
            else:
                assert x == y, (a, b)
