"""Scoring a decode grid: K hypothesis sets x U utterances in one htkamd_results_score call against K runs of the reference's HResults
(oracle/_ref/HResults, one core) over the same master label files.  Prints one JSON line.

    python tools/results_bench.py [--sets 16] [--utts 2000] [--maxlen 40] [--vocab 1000] [--reps 20]

The references are random word sequences of 1..maxlen words; hypothesis set k is every reference with edits at a rate that grows with k
(a grid point that recognises worse).  Timed: read_s, the library reading the K + 1 master label files into id arrays; one_call_s, the
call from id arrays to per-pair counts and per-set totals on the host (uploads, both kernels, downloads; a host clock around the call,
which ends in a stream synchronise), the median of --reps calls after one that warms the device up; kernels_ms, the device's events
around the two kernels in those calls; reference_s, the K HResults processes one after the other (each reads its files too, so compare
it with read_s + one_call_s).  same_totals: every set's H D S I N equal the reference's WORD: line."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from htk_amd import capi      # noqa: E402


def write_mlf(path, ext, seqs):
    with open(path, "w") as f:
        f.write("#!MLF!#\n")
        for u, s in enumerate(seqs):
            f.write('"*/u%05d.%s"\n%s.\n' % (u, ext, "".join(w + "\n" for w in s)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=16); ap.add_argument("--utts", type=int, default=2000); ap.add_argument("--maxlen", type=int, default=40)
    ap.add_argument("--vocab", type=int, default=1000); ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    words = ["w%04d" % k for k in range(a.vocab)]
    refs = [[words[k] for k in rng.integers(0, a.vocab, rng.integers(1, a.maxlen + 1))] for _ in range(a.utts)]
    with tempfile.TemporaryDirectory() as d:
        J = lambda n: os.path.join(d, n)      # noqa: E731
        open(J("list"), "w").write("".join(w + "\n" for w in words))
        write_mlf(J("ref.mlf"), "lab", refs)
        for k in range(a.sets):
            p = 0.05 + 0.3 * k / max(a.sets - 1, 1)
            hyps = []
            for r in refs:
                h = []
                for w in r:
                    x = rng.random()
                    if x < p / 3:
                        continue
                    h.append(words[rng.integers(0, a.vocab)] if x < 2 * p / 3 else w)
                    if x > 1 - p / 3:
                        h.append(words[rng.integers(0, a.vocab)])
                hyps.append(h or [r[0]])
            write_mlf(J("rec%02d.mlf" % k), "rec", hyps)
        t0 = time.perf_counter()
        res = capi.Results()
        rm = capi.Mlf(J("ref.mlf"))
        sets = []
        for k in range(a.sets):
            m = capi.Mlf(J("rec%02d.mlf" % k))
            sets.append([res.ids(h) for _, h in m.entries()])
        ri = [res.ref_for("u%05d.rec" % u, [rm])[0] for u in range(a.utts)]
        read_s = time.perf_counter() - t0
        call, kern = [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            out = res.score(ri, sets)
            t1 = time.perf_counter()
            if rep:
                call.append(t1 - t0); kern.append(out["kernel_ms"])
        labels = int(sum(len(h) for s in sets for h in s) + a.sets * sum(len(r) for r in refs))
        line = dict(sets=a.sets, utts=a.utts, pairs=a.sets * a.utts, labels=labels, read_s=round(read_s, 4), one_call_s=round(statistics.median(call), 5),
                    kernels_ms=round(statistics.median(kern), 3), kernel_share=round(statistics.median(kern) / 1000.0 / statistics.median(call), 3), reps=a.reps)
        exe = os.path.join(ROOT, "oracle", "_ref", "HResults")
        if os.path.exists(exe):
            same = True
            t0 = time.perf_counter()
            outs = [subprocess.run([exe, "-I", "ref.mlf", "list", "rec%02d.mlf" % k], cwd=d, check=True, stdout=subprocess.PIPE, text=True).stdout for k in range(a.sets)]
            line["reference_s"] = round(time.perf_counter() - t0, 4)
            for k, o in enumerate(outs):
                m = re.search(r"WORD: .*\[H=(\d+), D=(\d+), S=(\d+), I=(\d+), N=(\d+)\]", o)
                same = same and [int(x) for x in m.groups()] == out["totals"][k, :5].tolist()
            line["same_totals"] = same
        print(json.dumps(line))


if __name__ == "__main__":
    main()
