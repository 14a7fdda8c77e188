"""tests/golden/vq: the VQ tables the reference's HQuant wrote and the DISCRETE files its HCopy wrote from them.

    python tests/golden/make_vq_golden.py HQUANT HCOPY

HQUANT and HCOPY are the reference's tools, built outside the repository (HQuant is not among the tools of oracle/Makefile: the same
compiler line as its tools, HTKTools/HQuant.c against oracle/_ref/HTKLib.a).  The parameter files are random MFCC_D vectors (three
static and three delta columns, so that two streams split 3 + 3 as consecutive columns); b.mfc repeats rows, so equal distances occur.

    lin.vq   : HQuant -d -n 1 6                   lin.vq  a.mfc b.mfc      (linear, INVDIAGC, one stream of 6)
    tree.vq  : HQuant -f -t -s 2 -n 1 4 -n 2 2    tree.vq a.mfc b.mfc      (binary, FULLC, streams 3 + 3)
    lin_g.vq : HQuant -d -g -n 1 6                lin_g.vq a.mfc b.mfc     (-g: the global covariance in every node)
    *_a.dis  : HCopy -C {TARGETKIND = MFCC_D_V, VQTABLE = <table>, SAVEASVQ = T, NSTREAMS = <streams>} a.mfc <out>
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from htk_amd import capi  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vq")
MFCC_D = 6 + 0o400


def main(hquant, hcopy):
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261126)
    centres = rng.normal(0, 4, (7, 6))
    a = (centres[rng.integers(0, 7, 90)] + rng.normal(0, 1, (90, 6))).astype(np.float32)
    b = (centres[rng.integers(0, 7, 70)] + rng.normal(0, 1, (70, 6))).astype(np.float32)
    b[40:] = b[rng.integers(0, 40, 30)]
    capi.parm_write(os.path.join(OUT, "a.mfc"), a, 100000, MFCC_D)
    capi.parm_write(os.path.join(OUT, "b.mfc"), b, 100000, MFCC_D)
    files = [os.path.join(OUT, "a.mfc"), os.path.join(OUT, "b.mfc")]
    tables = {"lin": (["-d", "-n", "1", "6"], 1), "lin_g": (["-d", "-g", "-n", "1", "6"], 1), "tree": (["-f", "-t", "-s", "2", "-n", "1", "4", "-n", "2", "2"], 2)}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (sw, streams) in tables.items():
            tab = os.path.join(OUT, name + ".vq")
            subprocess.check_call([hquant] + sw + [tab] + files)
            if name == "lin_g":
                continue
            cfg = os.path.join(tmp, name + ".cfg")
            with open(cfg, "w") as f:
                f.write("TARGETKIND = MFCC_D_V\nVQTABLE = %s\nSAVEASVQ = T\nNSTREAMS = %d\n" % (tab, streams))
            subprocess.check_call([hcopy, "-C", cfg, files[0], os.path.join(OUT, name + "_a.dis")])


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
