"""Rescoring a batch of lattices: U decoder-sized lattices under K settings in one htkamd_latset_best call, against K runs of the
reference's HLRescore -f (oracle/_ref/HLRescore, one core) over the same files.  Prints one JSON line.

    python tools/latrescore_bench.py [--lats 2000] [--reps 20]

The lattices are the seeded random DAGs of tests/golden/make_latrescore_golden.py in the sizes the decoders give: 5-70 nodes, 1-3 arcs a
node -- `set_lattice_bench.py`'s alignment lattices have about 12 arcs each, the `-n 4` recognition fixtures 85-166.  Timed: read_s, the
library reading the files (with prep_s of it the orders: a second pass that re-adds every lattice through htkamd_latset_add_pruned, which
only copies and prepares); then for K = 1 and K = 16: one_call_s, the call from the prepared set to paths and totals on the host (uploads
of the scales, the kernel, downloads; a host clock around the call, which ends in a stream synchronise; the set's arrays are on the
device after the warm-up call), the median of --reps calls; kernels_ms, the device's events around the kernel; labels_s, the K x U label
lists written as master label files; reference_s, the K HLRescore -f -i processes one after the other (each reads the files too, so compare
it with read_s + one_call_s + labels_s).  same_labels: every master label file equals the reference's."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from htk_amd import capi      # noqa: E402
import make_latrescore_golden as gen      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lats", type=int, default=2000); ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rng = random.Random(5)
    grid = [(1.0, s, p, 1.0) for s in (1.0, 5.0, 10.0, 15.0) for p in (0.0, -5.0, -10.0, -20.0)]
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "in"))
        names = ["l%05d" % i for i in range(a.lats)]
        for n in names:
            nn = rng.randrange(5, 71)
            open(os.path.join(d, "in", n + ".lat"), "w").write(gen.random_lattice(rng, nn, rng.randrange(nn, 3 * nn), n, nn >= 8 and rng.random() < 0.3))
        open(os.path.join(d, "dict"), "w").write(gen.RAND_DICT)
        open(os.path.join(d, "cfg"), "w").write("STARTWORD = !SENT_START\nENDWORD = !SENT_END\n")
        t0 = time.perf_counter()
        ls = capi.LatSet(os.path.join(d, "dict"), "!SENT_START", "!SENT_END")
        for n in names:
            ls.add_file(os.path.join(d, "in", n + ".lat"))
        read_s = time.perf_counter() - t0
        nn, na = ls.sizes()
        t0 = time.perf_counter()
        copy = capi.LatSet(like=ls)
        L = capi.lib()
        ones = np.ones(int(max(nn.max(), na.max())), np.uint8)
        for u in range(len(ls)):
            L.htkamd_latset_add_pruned(copy.h, ls.h, u, capi._p(ones), capi._p(ones))
        prep_s = time.perf_counter() - t0
        line = dict(lats=a.lats, nodes=int(nn.sum()), arcs=int(na.sum()), read_s=round(read_s, 4), prep_s=round(prep_s, 4), reps=a.reps)
        exe = os.path.join(ROOT, "oracle", "_ref", "HLRescore")
        for K in (1, 16):
            st = grid[:K]
            call, kern = [], []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                out = ls.best(st)
                t1 = time.perf_counter()
                if rep:
                    call.append(t1 - t0); kern.append(out["kernel_ms"])
            t0 = time.perf_counter()
            for k in range(K):
                mlf = capi.MlfOut(os.path.join(d, "dev%d.mlf" % k))
                for u, n in enumerate(names):
                    mlf.add("in/%s.rec" % n, ls.trans(u, st[k], out["paths"][k][u]))
                mlf.close()
            labels_s = time.perf_counter() - t0
            r = dict(one_call_s=round(statistics.median(call), 5), kernels_ms=round(statistics.median(kern), 3),
                     kernel_share=round(statistics.median(kern) / 1000.0 / statistics.median(call), 3), labels_s=round(labels_s, 4))
            r["host_share_of_all"] = round(1.0 - statistics.median(kern) / 1000.0 / (read_s + statistics.median(call) + labels_s), 4)
            if os.path.exists(exe):
                t0 = time.perf_counter()
                for k in range(K):
                    subprocess.run([exe, "-C", "cfg", "-f", "-i", "ref%d.mlf" % k, "-a", str(st[k][0]), "-s", str(st[k][1]), "-p", str(st[k][2]), "-r", str(st[k][3]), "dict"] +
                                   ["in/%s.lat" % n for n in names], cwd=d, check=True, stdout=subprocess.DEVNULL)
                r["reference_s"] = round(time.perf_counter() - t0, 4)
                r["same_labels"] = all(open(os.path.join(d, "dev%d.mlf" % k)).read() == open(os.path.join(d, "ref%d.mlf" % k)).read() for k in range(K))
            line["K%d" % K] = r
        print(json.dumps(line))


if __name__ == "__main__":
    main()
