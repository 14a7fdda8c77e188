"""Wall time of tree-based state tying on a synthetic triphone set of a stated size: examples/tree_cluster.py (the device) and, where
oracle/_ref/HHEd exists, the reference's HHEd on the same files.  Prints one JSON line.

    python tools/tree_bench.py [--phones 40] [--contexts 600] [--dim 39] [--questions 200]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from htk_amd import capi


def write_inputs(d, P, NC, D, NQ, seed=1):
    rng = np.random.RandomState(seed)
    phones = ["p%02d" % k for k in range(P)]
    e = lambda v: " ".join("%e" % x for x in v)
    names = []
    with open(os.path.join(d, "hmmdefs"), "w") as f:
        f.write("~o\n<STREAMINFO> 1 %d\n<VECSIZE> %d<NULLD><USER><DIAGC>\n" % (D, D))
        f.write('~t "T"\n<TRANSP> 5\n 0 1 0 0 0\n 0 0.6 0.4 0 0\n 0 0 0.6 0.4 0\n 0 0 0 0.7 0.3\n 0 0 0 0 0\n')
        loff, roff = rng.randn(P, D), rng.randn(P, D)
        for c in phones:
            base = rng.randn(3, D) * 2
            seen = set()
            while len(seen) < min(NC, P * P):
                seen.add((rng.randint(P), rng.randint(P)))
            for l, r in sorted(seen):
                n = "%s-%s+%s" % (phones[l], c, phones[r]); names.append(n)
                f.write('~h "%s"\n<BEGINHMM>\n<NUMSTATES> 5\n' % n)
                for j in range(3):
                    var = 0.5 + rng.rand(D)
                    f.write("<STATE> %d\n<MEAN> %d\n %s\n<VARIANCE> %d\n %s\n" % (j + 2, D, e(base[j] + loff[l] * (1 - j / 2) + roff[r] * (j / 2) + rng.randn(D) * 0.3), D, e(var)))
                f.write('~t "T"\n<ENDHMM>\n')
    open(os.path.join(d, "hmmlist"), "w").write("\n".join(names) + "\n")
    mmf = capi.Mmf([os.path.join(d, "hmmdefs")], hmm_list=os.path.join(d, "hmmlist"))
    pk = mmf.packed(); lay = capi.accs_layout(pk)
    vec = np.zeros(lay.total)
    vec[lay.wtOcc:lay.wtOcc + pk["numStates"]] = 5 + rng.rand(pk["numStates"]) * 200
    vec[lay.nEgs:lay.nEgs + pk["numPhys"]] = 10
    capi.stats_write_file(pk, vec, mmf.phys_names, os.path.join(d, "stats"))
    lines = ["RO 100.0 stats"]
    for k in range(NQ):
        members = rng.choice(P, 1 + rng.randint(max(P // 3, 1)), replace=False)
        pat = "%s-*" if k % 2 == 0 else "*+%s"
        lines.append("QS 'Q%d' { %s }" % (k, ",".join('"%s"' % (pat % phones[m]) for m in members)))
    for c in phones:
        for j in (2, 3, 4):
            lines.append('TB 350.0 "ST_%s_%d_" {("*-%s+*").state[%d]}' % (c, j, c, j))
    lines.append("ST trees")
    open(os.path.join(d, "tree.hed"), "w").write("\n".join(lines) + "\n")
    return len(names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phones", type=int, default=40); ap.add_argument("--contexts", type=int, default=600)
    ap.add_argument("--dim", type=int, default=39); ap.add_argument("--questions", type=int, default=200)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        H = write_inputs(d, a.phones, a.contexts, a.dim, a.questions)
        res = dict(models=H, trees=3 * a.phones, questions=a.questions, dim=a.dim)
        t0 = time.time()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tree_cluster.py"), "tree.hed", "hmmdefs", "hmmlist", "stats", "-o", "tied_dev.mmf", "--trees", "trees_dev"],
                           cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        res["device_s"] = round(time.time() - t0, 3)
        if r.returncode:
            raise SystemExit("tree_cluster failed:\n" + r.stdout[-2000:])
        hhed = os.path.join(ROOT, "oracle", "_ref", "HHEd")
        if os.path.exists(hhed):
            t0 = time.time()
            subprocess.run([hhed, "-H", "hmmdefs", "-w", "tied_ref.mmf", "tree.hed", "hmmlist"], cwd=d, check=True, stdout=subprocess.DEVNULL)
            res["hhed_s"] = round(time.time() - t0, 3)
            res["identical"] = (open(os.path.join(d, "tied_dev.mmf"), "rb").read() == open(os.path.join(d, "tied_ref.mmf"), "rb").read()
                                and open(os.path.join(d, "trees_dev"), "rb").read() == open(os.path.join(d, "trees"), "rb").read())
        print(json.dumps(res))


if __name__ == "__main__":
    main()
