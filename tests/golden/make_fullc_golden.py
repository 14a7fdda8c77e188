#!/usr/bin/env python3
"""Full-covariance (FULLC) sets through the reference, written under tests/golden/fullc/.  Needs oracle/_ref (oracle/Makefile).

    seed          the demo's single-Gaussian monophones (tests/golden/demo/hmm_final, MFCC_E_D, D = 26) rewritten by THIS script as one
                  FULLC set: <FULLC> for <DIAGC>, <INVCOVAR> = diag(1/var) for every <VARIANCE>, no <GCONST> (the loader computes it)
    fullc_in      HERest -C cfg -w 3 -v 0.05 -u tmvw -t 2000.0 -T 1 -H seed -L demo/labels -M <dir> demo/bcplist demo/train/*.mfc
                  (one embedded pass: the off-diagonal terms are real afterwards), <dir>/seed renamed
    herest.log    the "average log prob" line of that pass
    fullc_resaved HHEd -H fullc_in -w fullc_resaved empty.hed demo/bcplist       (LoadHMMSet + SaveHMMSet: the text writer's answer)
    fullc_in_bin  HHEd -B -H fullc_in -w fullc_in_bin empty.hed demo/bcplist     (the binary form)
    outp_tr1.bin  ref_outp -C cfg -c -H fullc_in demo/bcplist demo/train/tr1.mfc outp_tr1.bin   (float[T][H][3] SOutP scores of the
                  MFCC_E_D rows; 0 where a model is shorter)
    rec_test/     HVite -C cfg -H fullc_in -l rec_test -w demo/monLattice -t 300.0 -p 5.0 -s 0.0 demo/bcpvocab demo/bcplist demo/test/*.mfc
    rec_align/    HVite -C cfg -H fullc_in -l rec_align -a -m -L demo/labels -t 150.0 demo/bcpvocab demo/bcplist demo/train/tr1.mfc tr2.mfc
cfg holds `TARGETKIND = MFCC_E_D`.

    python tests/golden/make_fullc_golden.py"""
import glob
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEMO = os.path.join(ROOT, "tests", "golden", "demo")
REF = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(ROOT, "tests", "golden", "fullc")
# HVite's switches for the two .rec sets (besides -C cfg -H fullc_in -l <dir>); tests/test_gpu_fullc.py runs tools/bin/hvite with the same
RECOGNISE = ["-w", os.path.join(DEMO, "monLattice"), "-t", "300.0", "-p", "5.0", "-s", "0.0"]
ALIGN = ["-a", "-m", "-L", os.path.join(DEMO, "labels"), "-t", "150.0"]


def to_fullc(text):
    """A DIAGC definition as text -> the same set with diagonal inverse covariances."""
    text = text.replace("<DIAGC>", "<FULLC>")
    text = re.sub(r"<GCONST>[^\n]*\n", "", text)

    def inv(m):
        var = [float(v) for v in m.group(2).split()]
        D = int(m.group(1))
        assert len(var) == D
        rows = []
        for j in range(D):                       # WriteTriMat's order: for j, for i >= j: m[i][j], a line per j
            rows.append("".join(" %e" % ((1.0 / var[j]) if i == j else 0.0) for i in range(j, D)))
        return "<INVCOVAR> %d\n%s\n" % (D, "\n".join(rows))
    return re.sub(r"<VARIANCE> (\d+)\n([^<]*)", inv, text)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    files = sorted(glob.glob(os.path.join(DEMO, "train", "*.mfc")))
    lst = os.path.join(DEMO, "bcplist")
    with tempfile.TemporaryDirectory() as d:
        seed = []
        for k, name in enumerate(open(lst).read().split()):
            t = open(os.path.join(DEMO, "hmm_final", name)).read()
            if k > 0:
                t = t[t.index("~h"):]            # the global options once
            seed.append(to_fullc(t))
        open(os.path.join(OUT, "seed"), "w").write("".join(seed))
        cfg = os.path.join(d, "cfg"); open(cfg, "w").write("TARGETKIND = MFCC_E_D\n")
        os.makedirs(os.path.join(d, "p1"))
        log = subprocess.run([os.path.join(REF, "HERest"), "-C", cfg, "-w", "3", "-v", "0.05", "-u", "tmvw", "-t", "2000.0", "-T", "1",
                              "-H", os.path.join(OUT, "seed"), "-L", os.path.join(DEMO, "labels"), "-M", os.path.join(d, "p1"), lst] + files,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
        shutil.copy(os.path.join(d, "p1", "seed"), os.path.join(OUT, "fullc_in"))
        keep = [l for l in log.splitlines() if "average log prob" in l]
        open(os.path.join(OUT, "herest.log"), "w").write("\n".join(keep) + "\n")
        hed = os.path.join(d, "empty.hed"); open(hed, "w").write("")
        subprocess.check_call([os.path.join(REF, "HHEd"), "-H", os.path.join(OUT, "fullc_in"), "-w", os.path.join(OUT, "fullc_resaved"), hed, lst])
        subprocess.check_call([os.path.join(REF, "HHEd"), "-B", "-H", os.path.join(OUT, "fullc_in"), "-w", os.path.join(OUT, "fullc_in_bin"), hed, lst])
        subprocess.check_call([os.path.join(REF, "ref_outp"), "-C", cfg, "-c", "-H", os.path.join(OUT, "fullc_in"), lst, os.path.join(DEMO, "train", "tr1.mfc"),
                               os.path.join(OUT, "outp_tr1.bin")])
        for sub, opts, fs in (("rec_test", RECOGNISE, sorted(glob.glob(os.path.join(DEMO, "test", "*.mfc")))),
                              ("rec_align", ALIGN, files[:2])):
            os.makedirs(os.path.join(OUT, sub), exist_ok=True)
            subprocess.check_call([os.path.join(REF, "HVite"), "-C", cfg, "-H", os.path.join(OUT, "fullc_in"), "-l", os.path.join(OUT, sub)] + opts +
                                  [os.path.join(DEMO, "bcpvocab"), lst] + fs)
    print(keep, sorted(os.listdir(OUT)))
