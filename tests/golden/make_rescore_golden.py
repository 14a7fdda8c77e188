"""Known answers for per-file lattice rescoring, HVite -w (no network name) -L dir -X lat (DoAlignment HVite.c:830 with loadNetworks):
the reference's HVite writes a lattice per utterance of the `bigram` case's system (-n 4 4 -z lat), then decodes every utterance against
ITS lattice with other scales, penalties and beams than the first pass.
    python tests/golden/make_rescore_golden.py        (needs oracle/_ref, i.e. `make -C oracle`)
Writes tests/golden/decode/rescore/{lat/u*.lat, feats.npz, expected.json}: data only.  Everything runs inside a scratch directory under
relative names, so the lattices' header lines (UTTERANCE= lmname= vocab=) name no directory."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
from htk_amd import synth  # noqa: E402
from make_decode_golden import sample  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
SRC = os.path.join(HERE, "decode", "bigram")
OUT = os.path.join(HERE, "decode", "rescore")
FIRST = "-n 4 4 -t 250.0"
SECOND = ["-s 3.0 -p -5.0", "-t 60.0 -s 0.5 -p 4.0 -r 2.0"]


def read_mlf(path):
    per, cur = {}, None
    for line in open(path).read().splitlines()[1:]:
        if line.startswith('"'):
            cur = os.path.basename(line.strip('"')).replace(".rec", ""); per[cur] = []
        elif line == ".":
            cur = None
        elif cur is not None:
            per[cur].append(line)
    return per


def main():
    if not os.path.exists(os.path.join(REF, "HVite")):
        sys.exit("needs oracle/_ref (make -C oracle)")
    rng = np.random.default_rng(411)
    s = synth.generate(30, 3, 12, 3, 80, 11, D=13)               # the model set of the loop / bigram cases
    pk = s.packed()
    prons = {"AB": [[0, 1], [0, 2]], "CD": [[3, 4, 5]], "E": [[6]], "F": [[7]], "G": [[8, 9]], "H": [[10]], "I": [[11]]}
    words = list(prons)
    feats = []
    for u in range(6):
        ph = []
        for k in rng.integers(0, len(words), size=4 + u % 3):
            alt = prons[words[k]]
            ph += alt[int(rng.integers(0, len(alt)))]
        feats.append(sample(pk, ph, rng, frames_per_state=3))
    os.makedirs(os.path.join(OUT, "lat"), exist_ok=True)
    expected = {}
    with tempfile.TemporaryDirectory() as d:
        for f in ("MMF", "dict", "hmmlist", "net.slf"):
            shutil.copy(os.path.join(SRC, f), os.path.join(d, f))
        for u, X in enumerate(feats):
            synth.write_htk_param(os.path.join(d, "u%d.mfc" % u), X, kind=9)
        open(os.path.join(d, "scp"), "w").write("".join("u%d.mfc\n" % u for u in range(len(feats))))
        open(os.path.join(d, "config"), "w").write("")
        os.makedirs(os.path.join(d, "lat"))
        hv = [os.path.join(REF, "HVite"), "-C", "config", "-H", "MMF", "-S", "scp"]
        subprocess.run(hv + ["-i", "first.mlf", "-l", "lat", "-z", "lat", "-w", "net.slf"] + FIRST.split() + ["dict", "hmmlist"], check=True, cwd=d,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        for u in range(len(feats)):
            shutil.copy(os.path.join(d, "lat", "u%d.lat" % u), os.path.join(OUT, "lat", "u%d.lat" % u))
        for opts in SECOND + ["-m " + SECOND[0]]:
            subprocess.run(hv + ["-i", "out.mlf", "-w", "-L", "lat", "-X", "lat"] + opts.split() + ["dict", "hmmlist"], check=True, cwd=d,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            expected[opts] = read_mlf(os.path.join(d, "out.mlf"))
            shutil.copy(os.path.join(d, "out.mlf"), os.path.join(OUT, "hvite__%s.mlf" % opts.replace(" ", "_")))
    np.savez_compressed(os.path.join(OUT, "feats.npz"), **{"u%d" % u: X for u, X in enumerate(feats)})
    json.dump(expected, open(os.path.join(OUT, "expected.json"), "w"), indent=1)
    for k, per in expected.items():
        print(k, {u: len(v) for u, v in per.items()})


if __name__ == "__main__":
    main()
