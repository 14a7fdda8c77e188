"""tests/golden/compv_full: the FULLC sets the reference's HCompV wrote from three short parameter files, over the whole files and over
the segments labelled S.

    python tests/golden/make_compv_full_golden.py [HCOMPV]

HCOMPV is the reference's tool (default oracle/_ref/HCompV, one of the tools of oracle/Makefile).  The parameter files are seeded random
MFCC vectors of 13 correlated columns around a column offset (a.mfc 110, b.mfc 90, c.mfc 100 frames); every file has a label file of S
and V segments, one S segment running past the file's end as HCompV clips it (LoadFile HCompV.c:468).  proto is a one-state FULLC
prototype with a unit inverse covariance.

    hcompv_all/proto : HCompV -m -M hcompv_all -S train.scp proto
    hcompv_lab/proto : HCompV -m -l S -L . -M hcompv_lab -S train.scp proto

With --measure (no HCOMPV needed) it prints the figure the end-to-end test's tolerance comes from: the largest difference, relative to
the largest entry, between a float32 restatement of AccVar / CalcCovs (HCompV.c:392-411, :261-297) in file order and the float64 one,
on these files, after the inversion -- and, where the golden sets exist, the same difference between them and the float64 one.
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from htk_amd import capi  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "compv_full")
D, MFCC, PERIOD = 13, 6, 100000
FILES = {"a": 110, "b": 90, "c": 100}
LABELS = {"a": [(0, 30, "S"), (30, 75, "V"), (75, 110, "S")], "b": [(0, 41, "V"), (41, 44, "S"), (44, 90, "V")], "c": [(0, 1, "S"), (1, 60, "V"), (60, 130, "S")]}


def segments(seg_label=None):
    """[(file, first, count)] as LoadFile walks them: whole files, or the label's cases with the end clipped to the file."""
    out = []
    for name, n in FILES.items():
        if seg_label is None:
            out.append((name, 0, n))
            continue
        for a, b, lab in LABELS[name]:      # the label's end is a time: frames a .. b inclusive, as :463-471 read it
            if lab == seg_label:
                e = min(b, n - 1)
                out.append((name, a, max(e - a + 1, 0)))
    return out


def restate(rows, dt):
    """AccVar and CalcCovs over `rows` in order with sums, products and divisions in `dt`; the inversion in double (CovInvert), then float32."""
    s, q = np.zeros(D, dt), np.zeros((D, D), dt)
    for x in rows.astype(dt):
        s += x
        q += np.outer(x, x)
    n = dt(len(rows))
    m = s / n
    cov = q / n - np.outer(m, m)
    return m.astype(np.float32), np.linalg.inv(cov.astype(np.float64)).astype(np.float32)


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


def measure():
    worst = 0.0
    for lab, sub in ((None, "hcompv_all"), ("S", "hcompv_lab")):
        rows = np.concatenate([capi.parm_read(os.path.join(OUT, f + ".mfc"))[0][a:a + n] for f, a, n in segments(lab)])
        m32, i32 = restate(rows, np.float32)
        m64, i64 = restate(rows, np.float64)
        figs = [rel(m32, m64), rel(i32, i64)]
        worst = max(worst, *figs)
        line = "%s: %d frames, float32 restatement against float64: mean %.3e, inverse covariance %.3e" % (sub, len(rows), figs[0], figs[1])
        ref = os.path.join(OUT, sub, "proto")
        if os.path.exists(ref):
            pk = capi.Mmf(files=[ref]).packed()
            il = np.tril_indices(D)
            line += "; the reference's set against float64: mean %.3e, inverse covariance %.3e" % (rel(pk["mean"][0], m64), rel(pk["invCov"][0], i64[il]))
        print(line)
    print("largest float32 / float64 difference: %.3e; allowed: %.3e" % (worst, 4 * worst))


def main(hcompv):
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261127)
    mix = rng.normal(0, 1, (D, D)) * 0.3 + np.diag(np.linspace(3.0, 1.0, D))
    off = rng.normal(0, 6, D)
    for name, n in FILES.items():
        capi.parm_write(os.path.join(OUT, name + ".mfc"), (rng.normal(0, 1, (n, D)) @ mix + off).astype(np.float32), PERIOD, MFCC)
        with open(os.path.join(OUT, name + ".lab"), "w") as f:
            f.write("".join("%d %d %s\n" % (a * PERIOD, b * PERIOD, lab) for a, b, lab in LABELS[name]))
    rows = ["".join(" %.1f" % (1.0 if j == i else 0.0) for j in range(i, D)) for i in range(D)]
    with open(os.path.join(OUT, "proto"), "w") as f:
        f.write("~o <VecSize> %d <MFCC>\n~h \"proto\"\n<BeginHMM>\n<NumStates> 3\n<State> 2\n<Mean> %d\n%s\n<InvCovar> %d\n%s\n"
                "<TransP> 3\n 0.0 1.0 0.0\n 0.0 0.6 0.4\n 0.0 0.0 0.0\n<EndHMM>\n" % (D, D, " 0.0" * D, D, "\n".join(rows)))
    scp = os.path.join(OUT, "train.scp")
    with open(scp, "w") as f:
        f.write("".join(name + ".mfc\n" for name in FILES))
    for sub, sw in (("hcompv_all", []), ("hcompv_lab", ["-l", "S", "-L", "."])):
        os.makedirs(os.path.join(OUT, sub), exist_ok=True)
        subprocess.check_call([hcompv, "-m"] + sw + ["-M", sub, "-S", "train.scp", "proto"], cwd=OUT)
    os.remove(scp)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--measure"]
    if "--measure" not in sys.argv:
        main(os.path.abspath(args[0]) if args else os.path.join(ROOT, "oracle", "_ref", "HCompV"))
    measure()
