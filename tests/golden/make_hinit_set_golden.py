#!/usr/bin/env python3
"""Known answers for htkamd_hinit's corners, from the reference's HInit (oracle/_ref/HInit), one call per model and run:
    HInit -i 10 [run's switches] -L labels -l X -o X -M out -T 1 proto/X f0 f1 f2
A synthetic corpus of three files (D = 4, USER kind) with three models: A with FIVE emitting states beside B and C with three (two
mixture components per state); every model has one token exactly as long as it has emitting states; the values are scaled by 30, so
that the printed log probabilities (five decimals) resolve 1e-6 of their size; dimension 3 has a spread of 0.3, and one component of
C's middle state is rare.  The runs:
    plain   defaults                      umv     -u mv (transitions and weights stay the prototype's)
    vfloor  -v 0.5 (binds on dimension 3)       wfloor  -w 9000 (floor 0.09: HInit carries it for discrete sets only, no weight moves)
    python tests/golden/make_hinit_set_golden.py  -> tests/golden/hinit_set/{data.npz, labels/f*.lab, proto/X, <run>/X, <run>.log}"""
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "hinit_set")
D = 4
MODELS = {"A": (5, 1), "B": (3, 2), "C": (3, 2)}            # emitting states, components per state
RUNS = {"plain": [], "umv": ["-u", "mv"], "vfloor": ["-v", "0.5"], "wfloor": ["-w", "9000"]}


def proto(name):
    ne, M = MODELS[name]
    N = ne + 2
    out = ['~o <VecSize> %d <USER> <StreamInfo> 1 %d' % (D, D), '~h "%s"' % name, "<BeginHMM>", "<NumStates> %d" % N]
    for s in range(2, N):
        out.append("<State> %d <NumMixes> %d" % (s, M))
        for m in range(M):
            out.append("<Mixture> %d %.4f" % (m + 1, 1.0 / M))
            out += ["<Mean> %d" % D, " ".join(["0.0"] * D), "<Variance> %d" % D, " ".join(["1.0"] * D)]
    out.append("<TransP> %d" % N)
    for i in range(N):
        row = [0.0] * N
        if i == 0:
            row[1] = 1.0
        elif i < N - 1:
            row[i], row[i + 1] = 0.6, 0.4
        out.append(" ".join("%.3e" % x for x in row))
    out.append("<EndHMM>")
    return "\n".join(out) + "\n"


def corpus():
    """three files; a file is tokens behind one another, each label [first frame, last frame + 1) * 100000 (HInit takes the frame at
    the end time with it: consecutive tokens share it)"""
    r = np.random.RandomState(31)
    centre = {n: 4.0 * r.randn(MODELS[n][0], D) for n in MODELS}
    files, labels = [], []
    for f in range(3):
        rows, labs, t = [], [], 0
        for k in range(6):
            for n in "ABC":
                ne = MODELS[n][0]
                L = ne if (f == 1 and k == 2) else ne * 3 + int(r.randint(0, 5))        # one token of exactly ne frames per model
                st = (np.arange(L) * ne) // L
                x = centre[n][st] + 0.3 * r.randn(L, D)
                x[:, 3] = centre[n][st, 3] + 0.01 * r.randn(L)
                if n != "A":                                                            # a second mode in every mixture state
                    x[::2, 0] += 2.5
                rows.append(x); labs.append((t, t + L - 1, n)); t += L
        X = (30.0 * np.concatenate(rows)).astype(np.float32)
        files.append(X); labels.append(labs)
    # C's middle state: a rare third of a mode, four frames far away in dimension 1
    hits = 0
    for f in range(3):
        for (a, b, n) in labels[f]:
            if n == "C" and hits < 4 and b - a + 1 >= 9:
                files[f][a + (b - a + 1) // 2, 1] += 270.0; hits += 1
    return files, labels


def write_param(path, X):
    with open(path, "wb") as f:
        f.write(struct.pack(">iihh", X.shape[0], 100000, X.shape[1] * 4, 9))
        f.write(np.ascontiguousarray(X, dtype=">f4").tobytes())


if __name__ == "__main__":
    hinit = os.path.join(ROOT, "oracle", "_ref", "HInit")
    if not os.path.exists(hinit):
        sys.exit("oracle/_ref/HInit is not built")
    files, labels = corpus()
    os.makedirs(os.path.join(OUT, "labels"), exist_ok=True); os.makedirs(os.path.join(OUT, "proto"), exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "data.npz"), **{"f%d" % i: X for i, X in enumerate(files)})
    for i, labs in enumerate(labels):
        open(os.path.join(OUT, "labels", "f%d.lab" % i), "w").write("".join("%d %d %s\n" % (a * 100000, b * 100000, n) for a, b, n in labs))
    for n in MODELS:
        open(os.path.join(OUT, "proto", n), "w").write(proto(n))
    with tempfile.TemporaryDirectory() as d:
        data = []
        for i, X in enumerate(files):
            data.append(os.path.join(d, "f%d.usr" % i)); write_param(data[-1], X)
        for run, sw in RUNS.items():
            os.makedirs(os.path.join(OUT, run), exist_ok=True)
            keep = []
            for n in MODELS:
                log = subprocess.run([hinit, "-i", "10"] + sw + ["-L", os.path.join(OUT, "labels"), "-l", n, "-o", n, "-M", os.path.join(OUT, run), "-T", "1",
                                      os.path.join(OUT, "proto", n)] + data, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
                for l in log.splitlines():
                    if re.search(r"Estimation (converged|aborted)|Iteration \d+: Average LogP|ERROR|WARNING", l):
                        keep.append("HInit %s: %s" % (n, l.strip()))
            open(os.path.join(OUT, run + ".log"), "w").write("\n".join(keep) + "\n")
            print(run); print("\n".join(keep))
