"""Known answers for N-best token sets and lattices with a network per file (DoAlignment -> ProcessFile, HVite.c:769-802, with nToks > 1):
the reference's HVite (built with -DPHNALG) rescoring the `rescore` fixture's lattices to new lattices and to N-best lists, and aligning the
`align` fixture's word transcriptions with several tokens, which gives the lattice of a known word sequence's pronunciation alternatives.
    python tests/golden/make_set_nbest_golden.py        (needs oracle/_ref, i.e. `make -C oracle`)
Reads the `bigram` system, rescore/{lat/u*.lat, feats.npz} and align/{feats.npz, words.json}; writes tests/golden/decode/set_nbest/
{index.json, <tag>/{out.mlf, u*.<ext>}}: data only.  Everything runs inside a scratch directory under relative names (features in r/ and
a/, first-pass lattices in lat/, outputs in out/), so the lattices' header lines name no directory but those."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from htk_amd import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
GOLD = os.path.join(HERE, "decode")
SRC, RESCORE, ALIGN = os.path.join(GOLD, "bigram"), os.path.join(GOLD, "rescore"), os.path.join(GOLD, "align")
OUT = os.path.join(GOLD, "set_nbest")
# tag: what the files are decoded against (a lattice per file / the file's word transcription), the decoder's switches, -n i [N], the
# lattice extension (-z) or None, the label switches
CASES = {
    "rescore_lat": dict(kind="rescore", opts="-s 3.0 -p -5.0", nToks=4, nTrans=1, latExt="lt2", lab=""),
    "rescore_nbest": dict(kind="rescore", opts="-t 200.0 -s 0.5 -p 4.0 -r 2.0", nToks=3, nTrans=3, latExt=None, lab=""),
    "rescore_u": dict(kind="rescore", opts="-t 250.0 -u 12 -s 3.0 -p -5.0", nToks=4, nTrans=1, latExt="lt2", lab=""),
    "align_lat": dict(kind="align", opts="-t 1000.0", nToks=3, nTrans=1, latExt="lat", lab=""),
    "align_nbest_m": dict(kind="align", opts="-t 1000.0", nToks=3, nTrans=2, latExt=None, lab="-m"),
    "align_lat_m": dict(kind="align", opts="-t 1000.0", nToks=3, nTrans=1, latExt="lat", lab="-m"),
}


def npz(path):
    z = np.load(path)
    return [z["u%d" % u] for u in range(len(z.files))]


def switches(c):
    """The reference's command line for the case, after the model and script switches (tests/test_gpu_decoder_set_nbest.py gives tools/bin/hvite the same)."""
    sw = ["-w", "-L", "lat", "-X", "lat"] if c["kind"] == "rescore" else ["-a", "-I", "words.mlf"]
    sw += ["-S", "r.scp" if c["kind"] == "rescore" else "a.scp", "-i", "out.mlf", "-l", "out", "-n", str(c["nToks"])] + ([str(c["nTrans"])] if c["nTrans"] > 1 else [])
    return sw + (["-z", c["latExt"]] if c["latExt"] else []) + c["lab"].split() + c["opts"].split()


def lay_out(d):
    """The scratch directory both HVites run in: the system, r/u*.mfc + lat/u*.lat, a/u*.mfc + words.mlf, out/."""
    for f in ("MMF", "dict", "hmmlist"):
        shutil.copy(os.path.join(SRC, f), os.path.join(d, f))
    for sub in ("r", "a", "lat", "out"):
        os.makedirs(os.path.join(d, sub))
    n = {}
    for sub, src in (("r", RESCORE), ("a", ALIGN)):
        feats = npz(os.path.join(src, "feats.npz"))
        for u, X in enumerate(feats):
            synth.write_htk_param(os.path.join(d, sub, "u%d.mfc" % u), X, kind=9)
        open(os.path.join(d, sub + ".scp"), "w").write("".join("%s/u%d.mfc\n" % (sub, u) for u in range(len(feats))))
        n[sub] = len(feats)
    for u in range(n["r"]):
        shutil.copy(os.path.join(RESCORE, "lat", "u%d.lat" % u), os.path.join(d, "lat", "u%d.lat" % u))
    with open(os.path.join(d, "words.mlf"), "w") as f:
        f.write("#!MLF!#\n")
        for u, seq in enumerate(json.load(open(os.path.join(ALIGN, "words.json")))):
            f.write('"*/u%d.lab"\n%s\n.\n' % (u, "\n".join(seq)))
    open(os.path.join(d, "config"), "w").write("")
    return n


def read_mlf(path):
    """{utterance: [alternative: [label lines]]}"""
    per, cur = {}, None
    for line in open(path).read().splitlines()[1:]:
        if line.startswith('"'):
            cur = os.path.basename(line.strip('"')).replace(".rec", ""); per[cur] = [[]]
        elif line == ".":
            cur = None
        elif line == "///":
            per[cur].append([])
        elif cur is not None:
            per[cur][-1].append(line)
    return per


def main():
    if not os.path.exists(os.path.join(REF, "HVite")):
        sys.exit("needs oracle/_ref (make -C oracle)")
    if os.path.exists(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    index = {}
    richer = both = 0
    for tag, c in CASES.items():
        with tempfile.TemporaryDirectory() as d:
            n = lay_out(d)["r" if c["kind"] == "rescore" else "a"]
            subprocess.run([os.path.join(REF, "HVite"), "-C", "config", "-H", "MMF"] + switches(c) + ["dict", "hmmlist"], check=True, cwd=d,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            os.makedirs(os.path.join(OUT, tag))
            shutil.copy(os.path.join(d, "out.mlf"), os.path.join(OUT, tag, "out.mlf"))
            per = read_mlf(os.path.join(d, "out.mlf"))
            # (-u: an utterance whose tokens the pruning takes before the final node has no entry and no lattice -- beside the others)
            assert sorted(per) == ["u%d" % u for u in range(n)] or ("-u" in c["opts"] and 0 < len(per) < n), (tag, sorted(per))
            for u in range(n if c["latExt"] else 0):
                if "u%d" % u not in per:
                    assert not os.path.exists(os.path.join(d, "out", "u%d.%s" % (u, c["latExt"]))), (tag, u)
                    continue
                name = "u%d.%s" % (u, c["latExt"])
                shutil.copy(os.path.join(d, "out", name), os.path.join(OUT, tag, name))
                text = open(os.path.join(d, "out", name)).read()
                nodes, arcs = (int(x) for x in re.search(r"N=(\d+) +L=(\d+)", text).groups())
                if c["kind"] == "rescore" and arcs > len(per["u%d" % u][0]) + 1:      # (the best path's words and the arc into the final node)
                    richer += 1
                if c["kind"] == "align" and arcs > nodes - 1 and re.search(r"W=AB +v=1", text) and re.search(r"W=AB +v=2", text):      # (not a chain)
                    both += 1
                assert ("d=:" in text) == (c["lab"] == "-m"), (tag, u)
            # (alignment: the alternatives of a lattice differ in pronunciations only, and TranscriptionFromLattice keeps one transcription per word
            # sequence -- WordMatch, HRec.c:2273-2277 -- so -a -n i N writes the best one alone)
            if c["nTrans"] > 1:
                assert all(len(a) == (1 if c["kind"] == "align" else c["nTrans"]) for a in per.values()), tag
            index[tag] = dict(c, n=n, nbest=per)
            print(tag, n, {u: len(a) for u, a in per.items()})
    # the fixtures are not trivial: a rescored lattice with more arcs than its best path has words, an alignment lattice with both pronunciations of AB
    assert richer > 0 and both > 0, (richer, both)
    json.dump(index, open(os.path.join(OUT, "index.json"), "w"), indent=1)
    print("richer rescored lattices:", richer, " alignment lattices with both pronunciations of AB:", both)


if __name__ == "__main__":
    main()
