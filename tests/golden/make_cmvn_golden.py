#!/usr/bin/env python3
"""Golden vectors for side-based cepstral mean and variance normalisation (CMEANDIR / CMEANMASK / CMEANPATHMASK, VARSCALEDIR /
VARSCALEMASK / VARSCALEPATHMASK / VARSCALEFN; HCompV -c -k -p -q) -- generated with the reference's own HCompV and HCopy (oracle/_ref,
built by oracle/Makefile) from HTKDemo's MFCC_E files under tests/golden/demo, copied under side-bearing names.

    python tests/golden/make_cmvn_golden.py

Writes tests/golden/cmvn/:
    data/<side>_<n>.mfc      copies of demo files: sides spa (3 utterances), spb (2), tpc (1) under the mask */%%%_*.mfc
    files.lst                their names
    cmn/<side>               HCompV -q nmv, TARGETKIND = MFCC_E_D_A
    cvn/<side>               HCompV -q nv, TARGETKIND = MFCC_E_D_A_Z with the side means applied (a variance file must carry the kind
                             it is applied to, HParm.c:3298: the files of the mean + variance case)
    cmn_p/<s>/<side>         HCompV -q nmv -p %??: the path mask's directory level
    varscale                 a <VARSCALE> vector written here by hand
    <case>.conf              the settings of a case, @GOLD@ standing for this directory
    out/<case>/<name>.htk    what HCopy wrote under <case>.conf: mean, var (target without _Z), both.  Under path.conf HCopy writes the
                             bytes of out/mean (the same means, found one directory level down): checked here, not kept twice
    README                   one line, with the reference's measured deviation from fp64 arithmetic
"""
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.path.join(ROOT, "oracle", "_ref")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")
OUT = os.path.join(ROOT, "tests", "golden", "cmvn")

FILES = [("spa_1", "train/tr1.mfc"), ("spa_2", "train/tr2.mfc"), ("spa_3", "train/tr3.mfc"), ("spb_1", "train/tr4.mfc"),
         ("spb_2", "train/tr5.mfc"), ("tpc_1", "test/te1.mfc")]
MASK = "*/%%%_*.mfc"
PATHMASK = "*/%??_*.mfc"
CASES = {
    "mean": "TARGETKIND = MFCC_E_D_A_Z\nCMEANDIR = @GOLD@/cmn\nCMEANMASK = %s\n" % MASK,
    "var": "TARGETKIND = MFCC_E_D_A\nVARSCALEDIR = @GOLD@/cmn\nVARSCALEMASK = %s\nVARSCALEFN = @GOLD@/varscale\n" % MASK,
    "both": "TARGETKIND = MFCC_E_D_A_Z\nCMEANDIR = @GOLD@/cmn\nCMEANMASK = %s\nVARSCALEDIR = @GOLD@/cvn\nVARSCALEMASK = %s\n"
            "VARSCALEFN = @GOLD@/varscale\n" % (MASK, MASK),
    "path": "TARGETKIND = MFCC_E_D_A_Z\nCMEANDIR = @GOLD@/cmn_p\nCMEANMASK = %s\nCMEANPATHMASK = %s\n" % (MASK, PATHMASK),
}


def read_htk(path):
    raw = open(path, "rb").read()
    n, _per, size, _kind = struct.unpack(">iihh", raw[:12])
    return np.frombuffer(raw[12:12 + n * size], ">f4").astype(np.float32).reshape(n, size // 4)


def read_side(path):
    tok = open(path).read().split()
    out = {"kind": tok[1][1:-1]}
    i = 2
    while i < len(tok):
        if tok[i] == "<NFRAMES>":
            out["n"] = int(tok[i + 1]); i += 2
        elif tok[i] in ("<MEAN>", "<VARIANCE>"):
            d = int(tok[i + 1])
            out[tok[i]] = np.array([float(t) for t in tok[i + 2:i + 2 + d]], np.float32); i += 2 + d
        else:
            i += 1
    return out


def conf(d, name, text):
    p = os.path.join(d, name)
    open(p, "w").write(text.replace("@GOLD@", OUT))
    return p


if __name__ == "__main__":
    shutil.rmtree(OUT, ignore_errors=True)
    for sub in ("data", "cmn", "cvn", "cmn_p/s", "cmn_p/t", "out"):
        os.makedirs(os.path.join(OUT, sub))
    names = []
    for name, src in FILES:
        shutil.copyfile(os.path.join(DEMO, src), os.path.join(OUT, "data", name + ".mfc"))
        names.append(os.path.join(OUT, "data", name + ".mfc"))
    open(os.path.join(OUT, "files.lst"), "w").write("".join("data/%s.mfc\n" % n for n, _ in FILES))
    vs = [0.5 + 0.37 * ((7 * i) % 13) for i in range(39)]                                # (b) a global variance vector, by hand
    open(os.path.join(OUT, "varscale"), "w").write("<VARSCALE> 39\n" + "".join(" %e" % v for v in vs) + "\n")
    with tempfile.TemporaryDirectory() as d:
        hcompv, hcopy = os.path.join(REF, "HCompV"), os.path.join(REF, "HCopy")
        plain = conf(d, "plain", "TARGETKIND = MFCC_E_D_A\n")
        # (a) the side statistics
        subprocess.check_call([hcompv, "-C", plain, "-c", os.path.join(OUT, "cmn"), "-k", MASK, "-q", "nmv"] + names, stdout=subprocess.DEVNULL)
        subprocess.check_call([hcompv, "-C", plain, "-c", os.path.join(OUT, "cmn_p"), "-k", MASK, "-p", "%??", "-q", "nmv"] + names, stdout=subprocess.DEVNULL)
        subprocess.check_call([hcompv, "-C", conf(d, "z", CASES["mean"]), "-c", os.path.join(OUT, "cvn"), "-k", MASK, "-q", "nv"] + names,
                              stdout=subprocess.DEVNULL)
        # (c), (d) the normalised files
        for case, text in CASES.items():
            open(os.path.join(OUT, case + ".conf"), "w").write(text)
            dst = os.path.join(d, "path_out") if case == "path" else os.path.join(OUT, "out", case)
            os.makedirs(dst)
            for name, _ in FILES:
                subprocess.check_call([hcopy, "-C", conf(d, case, text), os.path.join(OUT, "data", name + ".mfc"), os.path.join(dst, name + ".htk")])
                if case == "path":
                    assert open(os.path.join(dst, name + ".htk"), "rb").read() == open(os.path.join(OUT, "out", "mean", name + ".htk"), "rb").read()
        # the reference's own deviation from fp64 arithmetic: its float sums per utterance and side (HCompV.c:559-563, :621-625) and the
        # 7 digits of %e, against the fp64 mean and variance of the rows HCopy codes as MFCC_E_D_A
        devM = devV = 0.0
        rows = {}
        for name, _ in FILES:
            t = os.path.join(d, name + ".htk")
            subprocess.check_call([hcopy, "-C", plain, os.path.join(OUT, "data", name + ".mfc"), t])
            rows.setdefault(name[:3], []).append(read_htk(t).astype(np.float64))
        for side, xs in sorted(rows.items()):
            x = np.concatenate(xs)
            m = x.mean(0); v = (x * x).mean(0) - m * m
            ref = read_side(os.path.join(OUT, "cmn", side))
            assert ref["n"] == x.shape[0] and ref["kind"] == "MFCC_E_D_A"
            devM = max(devM, float(np.max(np.abs(ref["<MEAN>"] - m) / np.sqrt(v))))
            devV = max(devV, float(np.max(np.abs(ref["<VARIANCE>"] - v) / v)))
    line = ("Side-based CMN/CVN fixtures from the reference's HCompV / HCopy (make_cmvn_golden.py). The reference's own deviation from fp64 "
            "arithmetic on these files: means %.3g of a standard deviation, variances %.3g relative.\n" % (devM, devV))
    open(os.path.join(OUT, "README"), "w").write(line)
    print(line, end="")
    total = sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(OUT) for f in fs)
    print("%d bytes in %d files" % (total, sum(len(fs) for _, _, fs in os.walk(OUT))))
