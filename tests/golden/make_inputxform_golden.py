#!/usr/bin/env python3
"""Golden vectors for global linear input transforms (<INPUTXFORM> / ~j model sets, MATTRANFN files) -- generated with the reference's own
HCopy, HHEd, HVite and HERest (oracle/_ref, built by oracle/Makefile) from HTKDemo's MFCC_E files and labels under tests/golden/demo.

    python tests/golden/make_inputxform_golden.py

Writes tests/golden/inputxform/ (kept small: what the tests can derive from a committed file by moving or editing a few tokens they derive):
    data/{a,b,c}.mfc            MFCC_E statics: the first 9 frames of tr1, 33 of tr2 and ONE frame of tr3 (HCopy takes a one-frame file)
    xf/<name>                   transform files (~j "<name>" ...; what MATTRANFN names; full39 and exp45 in binary form, as the writer
                                restated in Python gives it, the others as text): full39 (39 x 39), proj20 (20 x 39), exp45 (45 x 39,
                                more rows than columns: the row grows, HParm.c:2207-2208), kind MFCC_E_D_A, applied after the qualifiers; for
                                TARGETKIND = MFCC_E_D_A_Z the same file with the kind MFCC_E_D_A_Z (HParm.c:1835: the kind must be the
                                qualified data's), made here and in the tests by editing the kind; pre13 (13 x 13 <PREQUAL>, kind MFCC_E,
                                serves both targets).  pre13b is pre13 with an <OFFSET> bias and a <LOGDET>, and pre13b.bin its binary form as
                                the writer restated in Python gives it (SaveInputXForm has no caller among the reference's tools that could
                                write it).  Seeded random entries of mixed sign and magnitude.
    out/<name>/<target>/<f>.htk what HCopy wrote under MATTRANFN, TARGETKIND = <target>: it DOES write tgtUsed = mrows columns
                                (HParm.c:3714-3723), 39 for pre13.  Checked here against the NumPy float32 restatement of ApplyStaticMat's
                                loop (tests/inputxform_util.py) in every bit before anything is kept: after the qualifiers on the rows HCopy
                                itself codes without a transform; <PREQUAL> on HCopy's own coding of the restated statics (as USER rows, whose
                                _Z takes the mean off every static: the reference's "do everything" rule, HParm.c:1716-1720).
    sets/inline.mmf             the demo's five models as a 20-dimensional single-Gaussian set (estimated here from the labelled frames of
                                the projected data) with <INPUTXFORM> proj20 inline, AS HHEd RE-SAVES IT (empty edit script); a second
                                re-save gives the same bytes, so the file is its own expected write-back.  inline_bin.mmf: HHEd -B.
    sets/macro_bin.mmf          the ~j form of the set in binary: the transform as a ~j macro, then the set with <INPUTXFORM> ~j "proj20",
                                which is inline_bin.mmf rearranged by tests/inputxform_util.py macro_form.  The text ~j form is inline.mmf
                                rearranged the same way, here and in the tests, and is not kept.  HHEd reads both, and its re-saves of
                                either, text and binary, are the bytes of inline.mmf / inline_bin.mmf (checked here): GetOption does not
                                count its own reference to a ~j macro, so PutOptions writes the transform in full and SaveMacros writes no
                                ~j (HModel.c:647, :3257, :4350) -- nor a second ~j macro that nobody names (checked here too).
    e2e/rec/<u>.rec             HVite -a -m -f of the untransformed demo files tr1 and tr3 through sets/inline.mmf (TARGETKIND = MFCC_E_D_A)
    e2e/wav_align.rec           HVite -a -m -f of tests/golden/wave/test.wav, coded by HVite itself (make_wav_labels_golden.py's case:
                                MFCC_0_D_A), through that case's fitted 39-dimensional set with xf/full39 (kind MFCC_0_D_A) as its
                                <INPUTXFORM>: the transform behind a waveform source
    e2e/herest.models, .log     the set one HERest iteration writes from the same files (-t 2000.0), from its first ~h on -- what stands
                                before it is inline.mmf's head byte for byte (checked here) --, and what HERest printed
"""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from inputxform_util import macro_form, wav_case_set, with_kind, xform_ref  # noqa: E402
import make_wav_labels_golden as wavcase  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
DEMO = os.path.join(HERE, "demo")
OUT = os.path.join(HERE, "inputxform")
CUTS = [("a", "tr1", 9), ("b", "tr2", 33), ("c", "tr3", 1)]
TARGETS = ["MFCC_E_D_A", "MFCC_E_D_A_Z"]
E2E = ["tr1", "tr3"]
SETID, MASK = "demo20", "demo*"


def read_htk(path):
    raw = open(path, "rb").read()
    n, per, size, kind = struct.unpack(">iihh", raw[:12])
    return np.frombuffer(raw[12:12 + n * size], ">f4").astype(np.float32).reshape(n, size // 4)


def write_htk(path, X, kind):
    with open(path, "wb") as f:
        f.write(struct.pack(">iihh", X.shape[0], 100000, X.shape[1] * 4, kind))
        f.write(np.ascontiguousarray(X, ">f4").tobytes())


def matrix(rng, r, c):
    m = rng.normal(0.0, 1.0, (r, c)) * 10.0 ** rng.uniform(-2.5, 0.5, (r, c))
    return np.array([[np.float32("%e" % v) for v in row] for row in m], np.float32)      # the values a text file holds


def fvec(v):
    return "".join(" %e" % x for x in v)


def xform_body(mask, kind, prequal, M, bias=None, logdet=0.0):
    s = "<MMFIDMASK> %s <%s>%s\n<LINXFORM><VECSIZE> %d\n" % (mask, kind, "<PREQUAL>" if prequal else "", M.shape[0])
    if bias is not None:
        s += "<OFFSET>\n<BIAS> %d\n%s\n" % (len(bias), fvec(bias))
    if logdet:
        s += "<LOGDET> %e\n" % logdet
    s += "<BLOCKINFO> 1 %d\n<BLOCK> 1\n<XFORM> %d %d\n" % (M.shape[0], M.shape[0], M.shape[1])
    return s + "".join(fvec(row) + "\n" for row in M)


def xform_binary(name, mask, kind, prequal, M, bias, logdet):
    """SaveInputXForm(binary = TRUE) restated: ':' + code byte keywords (enum Symbol HModel.c:394-411), big-endian ints / shorts / floats"""
    sym = lambda c: b":" + bytes([c])
    b = ('~j "%s"' % name).encode() + sym(104) + (" %s <%s>" % (mask, kind)).encode() + (sym(108) if prequal else b"")
    b += sym(94) + sym(6) + struct.pack(">i", M.shape[0])
    if bias is not None:
        b += sym(95) + sym(96) + struct.pack(">h", len(bias)) + np.asarray(bias, ">f4").tobytes()
    if logdet:
        b += sym(97) + struct.pack(">f", logdet)
    b += sym(98) + struct.pack(">ii", 1, M.shape[0]) + sym(99) + struct.pack(">i", 1) + sym(23) + struct.pack(">hh", *M.shape)
    return b + np.asarray(M, ">f4").tobytes()


def hcopy(conf_text, src, dst, d):
    conf = os.path.join(d, "hcopy.conf")
    open(conf, "w").write(conf_text)
    subprocess.check_call([os.path.join(REF, "HCopy"), "-C", conf, src, dst])
    return read_htk(dst)


def model_set(stats, D, xf_text, macro_text=""):
    s = macro_text + "~o\n<HMMSETID> %s\n<STREAMINFO> 1 %d\n<VECSIZE> %d<NULLD><MFCC_E_D_A><DIAGC>\n%s" % (SETID, D, D, xf_text)
    for name in "SCVNL":
        s += '~h "%s"\n<BEGINHMM>\n<NUMSTATES> 5\n' % name
        for j in range(3):
            mu, var = stats[name][j]
            s += "<STATE> %d\n<MEAN> %d\n%s\n<VARIANCE> %d\n%s\n" % (j + 2, D, fvec(mu), D, fvec(var))
        s += "<TRANSP> 5\n 0 1 0 0 0\n 0 0.6 0.4 0 0\n 0 0 0.6 0.4 0\n 0 0 0 0.7 0.3\n 0 0 0 0 0\n<ENDHMM>\n"
    return s


def main():
    shutil.rmtree(OUT, ignore_errors=True)
    for sub in ("data", "xf", "out", "sets", "e2e/rec"):
        os.makedirs(os.path.join(OUT, sub))
    rng = np.random.default_rng(20261018)
    mats = {"full39": matrix(rng, 39, 39), "proj20": matrix(rng, 20, 39), "pre13": matrix(rng, 13, 13), "exp45": matrix(rng, 45, 39)}
    kinds = {"full39": "MFCC_E_D_A", "proj20": "MFCC_E_D_A", "exp45": "MFCC_E_D_A", "pre13": "MFCC_E"}
    for name, M in mats.items():
        if name in ("full39", "exp45"):      # the two large ones in binary form: HCopy reads what the Python restatement of the writer wrote
            open(os.path.join(OUT, "xf", name), "wb").write(xform_binary(name, "*", kinds[name], False, M, None, 0.0))
        else:
            open(os.path.join(OUT, "xf", name), "w").write('~j "%s"\n' % name + xform_body("*", kinds[name], name == "pre13", M))
    bias = np.array([np.float32("%e" % v) for v in rng.normal(0, 2, 13)], np.float32)
    open(os.path.join(OUT, "xf", "pre13b"), "w").write('~j "pre13b"\n' + xform_body(MASK, "MFCC_E", True, mats["pre13"], bias, -3.25))
    open(os.path.join(OUT, "xf", "pre13b.bin"), "wb").write(xform_binary("pre13b", MASK, "MFCC_E", True, mats["pre13"], bias, -3.25))
    for name, src, n in CUTS:
        write_htk(os.path.join(OUT, "data", name + ".mfc"), read_htk(os.path.join(DEMO, "train", src + ".mfc"))[:n], 6 | 0o100)
    with tempfile.TemporaryDirectory() as d:
        # ---- HCopy under MATTRANFN, each file checked against the restatement
        nbits = 0
        for name, M in mats.items():
            for tgt in TARGETS:
                dst = os.path.join(OUT, "out", name, tgt)
                os.makedirs(dst)
                fn = os.path.join(OUT, "xf", name)
                if tgt.endswith("_Z") and name != "pre13":      # the same matrix under the kind of the _Z rows (the file's name is the macro's)
                    os.makedirs(os.path.join(d, "z"), exist_ok=True)
                    fn = with_kind(os.path.join(OUT, "xf", name), os.path.join(d, "z", name))
                for f, _, n in CUTS:
                    src = os.path.join(OUT, "data", f + ".mfc")
                    got = hcopy("TARGETKIND = %s\nMATTRANFN = %s\n" % (tgt, fn), src, os.path.join(dst, f + ".htk"), d)
                    if name == "pre13":
                        t = os.path.join(d, "pre.user")
                        write_htk(t, xform_ref(M, read_htk(src)), 9)
                        want = hcopy("TARGETKIND = %s\n" % tgt.replace("MFCC_E", "USER"), t, os.path.join(d, "pre.out"), d)
                    else:
                        want = xform_ref(M, hcopy("TARGETKIND = %s\n" % tgt, src, os.path.join(d, "plain.out"), d))
                    assert got.shape == (n, 39 if name == "pre13" else M.shape[0]), (name, tgt, f, got.shape)
                    assert got.tobytes() == want.tobytes(), "HCopy and the restatement differ: %s %s %s" % (name, tgt, f)
                    nbits += got.size
        print("HCopy == NumPy restatement in every bit: %d values" % nbits)
        # ---- the 20-dimensional set: per model and state the mean / variance of the labelled frames of the projected data
        proj = {}
        for u in E2E:
            proj[u] = hcopy("TARGETKIND = MFCC_E_D_A\nMATTRANFN = %s\n" % os.path.join(OUT, "xf", "proj20"), os.path.join(DEMO, "train", u + ".mfc"),
                            os.path.join(d, u + ".p20"), d)
        frames = {n: [[], [], []] for n in "SCVNL"}
        for u in E2E:
            for line in open(os.path.join(DEMO, "labels", u + ".lab")):
                a, b, n = line.split()
                seg = proj[u][int(round(int(a) / 1e5)):max(int(round(int(b) / 1e5)), int(round(int(a) / 1e5)) + 1)]
                for j, part in enumerate(np.array_split(seg, 3)):
                    frames[n][j].append(part)
        allv = np.concatenate(list(proj.values())).astype(np.float64).var(0)
        stats = {}
        for n in "SCVNL":
            stats[n] = []
            for j in range(3):
                x = np.concatenate(frames[n][j]).astype(np.float64)
                stats[n].append((x.mean(0), np.maximum(x.var(0), 0.05 * allv)))
        body = xform_body(MASK, "MFCC_E_D_A", False, mats["proj20"])
        sets = os.path.join(OUT, "sets")
        hhed = os.path.join(REF, "HHEd")
        shutil.copyfile(os.path.join(DEMO, "bcplist"), os.path.join(sets, "hmmlist"))
        open(os.path.join(d, "empty.hed"), "w").close()
        open(os.path.join(d, "first.mmf"), "w").write(model_set(stats, 20, "<INPUTXFORM>\n" + body))
        resave = lambda src, dst, *flag: subprocess.check_call([hhed, *flag, "-H", src, "-w", dst, os.path.join(d, "empty.hed"), "hmmlist"], cwd=sets)
        resave(os.path.join(d, "first.mmf"), "inline.mmf")
        resave("inline.mmf", "inline_bin.mmf", "-B")
        inline = open(os.path.join(sets, "inline.mmf")).read()
        head = inline[:inline.index("~h ")]
        open(os.path.join(d, "macro.mmf"), "w").write("".join(macro_form(inline)))
        open(os.path.join(sets, "macro_bin.mmf"), "wb").write(b"".join(macro_form(open(os.path.join(sets, "inline_bin.mmf"), "rb").read())))
        macro, rest = macro_form(inline)                                          # a second ~j macro that nobody names
        open(os.path.join(d, "extra.mmf"), "w").write(macro + macro.replace('"proj20"', '"unused"') + rest)
        for src in ("inline.mmf", os.path.join(d, "macro.mmf"), "macro_bin.mmf", os.path.join(d, "extra.mmf")):      # every re-save, of either form, is inline.mmf / inline_bin.mmf
            resave(src, os.path.join(d, "again.mmf")); resave(src, os.path.join(d, "again_bin.mmf"), "-B")
            assert open(os.path.join(d, "again.mmf"), "rb").read() == inline.encode(), src
            assert open(os.path.join(d, "again_bin.mmf"), "rb").read() == open(os.path.join(sets, "inline_bin.mmf"), "rb").read(), src
        # ---- HVite -a and one HERest iteration through the transformed set, from the untransformed files
        conf = os.path.join(d, "e2e.conf")
        open(conf, "w").write("TARGETKIND = MFCC_E_D_A\n")
        files = [os.path.join(DEMO, "train", u + ".mfc") for u in E2E]
        subprocess.check_call([os.path.join(REF, "HVite"), "-C", conf, "-H", os.path.join(sets, "inline.mmf"), "-a", "-m", "-f", "-L", os.path.join(DEMO, "labels"),
                               "-l", os.path.join(OUT, "e2e", "rec"), os.path.join(DEMO, "bcpvocab"), os.path.join(sets, "hmmlist")] + files)
        # ---- the same from a WAVEFORM: the 39-dimensional set fitted to tests/golden/wave/test.wav, behind the 39 x 39 transform
        wd = os.path.join(d, "wav"); os.makedirs(wd)
        open(os.path.join(wd, "xf.mmf"), "w").write(wav_case_set(open(os.path.join(HERE, "wave", "fitted.mmf")).read(),
                                                                 " ~j \"full39\"\n"))
        with_kind(os.path.join(OUT, "xf", "full39"), os.path.join(wd, "full39"), new="<MFCC_0_D_A>")
        open(os.path.join(wd, "inl.mmf"), "w").write(wav_case_set(open(os.path.join(HERE, "wave", "fitted.mmf")).read(),
                                                                  "\n" + xform_body("*", "MFCC_0_D_A", False, mats["full39"])))
        wavcase.write_case(wd, "WAV", mmf=os.path.join(wd, "inl.mmf"))
        lines = wavcase.run_tool(os.path.join(REF, "HVite"), wd, os.path.join(HERE, "wave", "test.wav"), "align")
        plain = os.path.join(d, "plainwav"); os.makedirs(plain); wavcase.write_case(plain, "WAV")
        assert lines != wavcase.run_tool(os.path.join(REF, "HVite"), plain, os.path.join(HERE, "wave", "test.wav"), "align")      # the transform shows
        open(os.path.join(OUT, "e2e", "wav_align.rec"), "w").write("".join(l + "\n" for l in lines))
        os.makedirs(os.path.join(d, "new"))
        log = subprocess.run([os.path.join(REF, "HERest"), "-C", conf, "-H", os.path.join(sets, "inline.mmf"), "-M", os.path.join(d, "new"), "-L", os.path.join(DEMO, "labels"),
                              "-t", "2000.0", "-T", "1", os.path.join(sets, "hmmlist")] + files, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
        new = open(os.path.join(d, "new", "inline.mmf")).read()
        assert new[:new.index("~h ")] == head and "WARNING" not in log, log
        open(os.path.join(OUT, "e2e", "herest.models"), "w").write(new[new.index("~h "):])
        open(os.path.join(OUT, "e2e", "herest.log"), "w").write("".join(l + "\n" for l in log.splitlines() if "HERest" not in l and d not in l))
    total = sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(OUT) for f in fs)
    print("%d bytes in %d files" % (total, sum(len(fs) for _, _, fs in os.walk(OUT))))


if __name__ == "__main__":
    main()
