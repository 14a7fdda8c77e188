"""Label statistics and network building timed: one htkamd_lstats_count + bigram file + back-off network + SLF against the reference's
HLStats -o -b followed by HBuild -n on one host core (oracle/_ref, when built), over a synthetic corpus with a Zipf-like word distribution.

    python tools/lm_bench.py [--labels 10000000] [--words 60000] [--utt-len 20] [--dir DIR] [--no-ref]

Prints one JSON line: kernel time, call time (upload, kernels, download), the host arithmetic and writers, the time spent reading the label
file into id arrays, the reference's wall time, and same_bytes (bigram file and SLF equal to the reference's)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", type=int, default=10_000_000)
    ap.add_argument("--words", type=int, default=60_000)
    ap.add_argument("--utt-len", type=int, default=20)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="lm_bench_")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(1)
    words = ["w%05d" % i for i in range(a.words)]
    p = 1.0 / np.arange(1, a.words + 1) ** 1.05
    draw = rng.choice(a.words, a.labels, p=p / p.sum()).astype(np.int32)
    n_utt = max(a.labels // a.utt_len, 1)
    bounds = np.linspace(0, a.labels, n_utt + 1).astype(np.int64)
    wl, mlf = os.path.join(d, "wordlist"), os.path.join(d, "labels.mlf")
    open(wl, "w").write("".join(w + "\n" for w in words))
    with open(mlf, "w") as f:
        f.write("#!MLF!#\n")
        for u in range(n_utt):
            f.write('"*/u%07d.lab"\n' % u + "".join(words[i] + "\n" for i in draw[bounds[u]:bounds[u + 1]]) + ".\n")
    res = dict(labels=a.labels, words=a.words, utterances=n_utt)

    t0 = time.perf_counter()
    ls = capi.LabelStats(words)
    table = {w: ls.id(w) for w in words}
    utts, cur = [], None
    for line in open(mlf):
        line = line.rstrip("\n")
        if line.startswith('"'):
            cur = []
        elif line == ".":
            utts.append(np.array(cur, np.int32))
        elif not line.startswith("#"):
            cur.append(table.get(line, 0))
    res["read_s"] = time.perf_counter() - t0
    ls.count(utts[:1])                                        # the first call loads the code object
    t0 = time.perf_counter()
    ls.count(utts)
    res["call_s"] = time.perf_counter() - t0
    res["kernel_ms"] = ls.kernel_ms
    t0 = time.perf_counter()
    ls.bigram_write(os.path.join(d, "ours.bo"), backoff=True)
    res["bigram_write_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    lm = capi.Bigram(os.path.join(d, "ours.bo"))
    res["bigram_read_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    net = capi.Network.from_bigram(lm, words + ["!ENTER", "!EXIT"])
    res["netbuild_s"], res["netbuild_kernel_ms"] = time.perf_counter() - t0, net.kernel_ms
    t0 = time.perf_counter()
    net.write(os.path.join(d, "ours.slf"))
    res["slf_write_s"] = time.perf_counter() - t0

    ref = os.path.join(ROOT, "oracle", "_ref")
    if not a.no_ref and os.path.exists(os.path.join(ref, "HLStats")):
        wl2 = os.path.join(d, "wordlist2")
        open(wl2, "w").write("".join(w + "\n" for w in words + ["!ENTER", "!EXIT"]))
        t0 = time.perf_counter()
        subprocess.run([os.path.join(ref, "HLStats"), "-o", "-b", os.path.join(d, "ref.bo"), wl, mlf], check=True)
        res["ref_hlstats_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        subprocess.run([os.path.join(ref, "HBuild"), "-n", os.path.join(d, "ref.bo"), wl2, os.path.join(d, "ref.slf")], check=True)
        res["ref_hbuild_s"] = time.perf_counter() - t0
        same = lambda x, y: open(os.path.join(d, x), "rb").read() == open(os.path.join(d, y), "rb").read()
        res["same_bytes"] = bool(same("ours.bo", "ref.bo") and same("ours.slf", "ref.slf"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
