#!/usr/bin/env python3
"""Known answers for htkamd_hrest's corners, from the reference's HRest (oracle/_ref/HRest), one call per model and run:
    HRest -T 1 -i 10 [run's switches] -L labels -l X -M out start/X f0 f1 f2
The corpus is tests/golden/hinit_set's (make_hinit_set_golden.py: three files, D = 4, USER kind; model A with FIVE emitting states, B
and C with three and two components per state; values scaled by 30 so that the five printed decimals resolve 1e-6 of the log
probability; dimension 3 has a spread of 0.3; one component of C's middle state is rare).  The starting models are what the reference's
HInit wrote for it (tests/golden/hinit_set/plain), copied to start/.  The runs:
    plain    defaults                               umv      -u mv (transitions and weights are not re-estimated)
    vfloor   -v 0.5 (binds on dimension 3)          wfloor   -w 9000 (floor 0.09: moves the rare component's weight)
    short    model A with labels_short/ (one token of A cut to three frames): dropped by default, kept and skipped with -t (short_t)
    few      model C with labels_few/ (two tokens of C left) and -m 3: HError 2221
    mix      the demo's mixture models: tests/golden/demo/hinit_mix/hmm0 -> HRest -i 10 -v 0.05 -w 3 (TARGETKIND = MFCC_E_D) -> mix/X
    python tests/golden/make_hrest_set_golden.py  -> tests/golden/hrest_set/{start/X, labels_short, labels_few, <run>/X, <run>.log}"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_hinit_set_golden import write_param  # noqa: E402

HSET = os.path.join(ROOT, "tests", "golden", "hinit_set")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")
OUT = os.path.join(ROOT, "tests", "golden", "hrest_set")
RUNS = {"plain": [], "umv": ["-u", "mv"], "vfloor": ["-v", "0.5"], "wfloor": ["-w", "9000"]}
KEEP = r"Estimation (converged|aborted)|Ave LogProb at iter|Examples loaded|ERROR|WARNING"


def read_labels(i):
    return [l.split() for l in open(os.path.join(HSET, "labels", "f%d.lab" % i))]


def write_labels(d, i, rows):
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "f%d.lab" % i), "w").write("".join("%s %s %s\n" % tuple(r) for r in rows))


def run(hrest, name, switches, labdir, start, out, data, conf=None):
    os.makedirs(out, exist_ok=True)
    cmd = [hrest, "-T", "1", "-i", "10"] + switches + (["-C", conf] if conf else []) + ["-L", labdir, "-l", name, "-M", out, os.path.join(start, name)] + data
    log = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    return ["HRest %s: %s" % (name, l.strip()) for l in log.splitlines() if re.search(KEEP, l) and "Terminating program" not in l]


if __name__ == "__main__":
    hrest = os.path.join(ROOT, "oracle", "_ref", "HRest")
    if not os.path.exists(hrest):
        sys.exit("oracle/_ref/HRest is not built")
    z = np.load(os.path.join(HSET, "data.npz"))
    os.makedirs(os.path.join(OUT, "start"), exist_ok=True)
    for n in "ABC":
        shutil.copy(os.path.join(HSET, "plain", n), os.path.join(OUT, "start", n))
    # short: the first token of A in f0 that is longer than five frames keeps its first three (end = start + 2 frames)
    cut = False
    for i in range(3):
        rows = read_labels(i)
        for r in rows:
            if not cut and i == 0 and r[2] == "A" and int(r[1]) - int(r[0]) >= 5 * 100000:
                r[1] = str(int(r[0]) + 2 * 100000); cut = True
        write_labels(os.path.join(OUT, "labels_short"), i, rows)
    # few: two tokens of C stay, the others are relabelled X (no model of that name: nobody's token)
    left = 2
    for i in range(3):
        rows = read_labels(i)
        for r in rows:
            if r[2] == "C":
                if left > 0:
                    left -= 1
                else:
                    r[2] = "X"
        write_labels(os.path.join(OUT, "labels_few"), i, rows)
    start = os.path.join(OUT, "start")
    with tempfile.TemporaryDirectory() as d:
        data = []
        for i in range(3):
            data.append(os.path.join(d, "f%d.usr" % i)); write_param(data[-1], z["f%d" % i])
        logs = {}
        for name, sw in RUNS.items():
            logs[name] = sum([run(hrest, n, sw, os.path.join(HSET, "labels"), start, os.path.join(OUT, name), data) for n in "ABC"], [])
        logs["short"] = run(hrest, "A", [], os.path.join(OUT, "labels_short"), start, os.path.join(OUT, "short"), data)
        logs["short_t"] = run(hrest, "A", ["-t"], os.path.join(OUT, "labels_short"), start, os.path.join(OUT, "short_t"), data)
        logs["few"] = run(hrest, "C", ["-m", "3"], os.path.join(OUT, "labels_few"), start, os.path.join(d, "few"), data)
        conf = os.path.join(d, "hrest.conf")
        open(conf, "w").write("TARGETKIND = MFCC_E_D\nSAVEGLOBOPTS = TRUE\nKEEPDISTINCT=F\n")
        train = sorted(glob.glob(os.path.join(DEMO, "train", "tr*.mfc")))
        logs["mix"] = sum([run(hrest, n, ["-v", "0.05", "-w", "3", "-D"], os.path.join(DEMO, "labels"), os.path.join(DEMO, "hinit_mix", "hmm0"),
                               os.path.join(OUT, "mix"), train, conf) for n in "SCVNL"], [])
    for name, keep in logs.items():
        open(os.path.join(OUT, name + ".log"), "w").write("\n".join(keep) + "\n")
        print(name); print("\n".join(keep))
