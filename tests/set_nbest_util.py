"""What the two test files of N-best decoding with a network per utterance share (tests/golden/decode/set_nbest, written by
tests/golden/make_set_nbest_golden.py): the fixture's cases as networks, features and decoder parameters, and the comparison of a lattice
with the files the reference's HVite wrote for it."""
import json
import os

import numpy as np

from decode_util import GOLD, parse_opts

SRC, ALIGN, RESCORE, SETNB = (os.path.join(GOLD, d) for d in ("bigram", "align", "rescore", "set_nbest"))
INDEX = json.load(open(os.path.join(SETNB, "index.json")))
TAGS = list(INDEX)


def npz(path):
    z = np.load(path)
    return [z["u%d" % u] for u in range(len(z.files))]


def bigram_mmf(native):
    return native.Mmf(files=[os.path.join(SRC, "MMF")], hmm_list=os.path.join(SRC, "hmmlist"))


def load_case(native, mmf, tag):
    """(case, networks -- one per utterance --, features, decoder parameters, alignment mode)."""
    c = INDEX[tag]
    dic = os.path.join(SRC, "dict")
    if c["kind"] == "rescore":
        feats = npz(os.path.join(RESCORE, "feats.npz"))
        nets = [native.Net(os.path.join(RESCORE, "lat", "u%d.lat" % u), dic, mmf) for u in range(len(feats))]
    else:
        feats = npz(os.path.join(ALIGN, "feats.npz"))
        nets = [native.Net(None, dic, mmf, words=w) for w in json.load(open(os.path.join(ALIGN, "words.json")))]
    assert len(feats) == c["n"]
    return c, nets, feats, parse_opts(c["opts"]), (1 if "-m" in c["lab"].split() else 0)


def with_prons(lat, net):
    """An oracle lattice with the fields the product's host code reads: nodePron, alModel, the scales."""
    a = net.arrays()
    lat = dict(lat)
    lat["nodePron"] = np.array([a["model"][n] if n >= 0 else -1 for n in lat["nodeNet"]], np.int32)
    if "alNode" in lat:
        lat["alModel"] = np.array([a["model"][n] for n in lat["alNode"]], np.int32)
    return lat


def word_labels(alt, net, frame_dur=100000):
    return ["%d %d %s %f" % (s * frame_dur, e * frame_dur, net.out_syms[w], np.float32(sc)) for w, s, e, sc in alt if w >= 0 and net.out_syms[w] != ""]


def check_files(native, lat, net, mmf, tag, u, tmp_path):
    """htkamd_lattice_write of `lat` is the file HVite wrote for utterance u, byte for byte (a lattice made in DoAlignment has no lmname
    line); the alternatives' label lines are those of HVite's label file."""
    c = INDEX[tag]
    align = 1 if "-m" in c["lab"].split() else 0
    if c["latExt"]:
        out = str(tmp_path / ("%s_u%d.%s" % (tag, u, c["latExt"])))
        native.lattice_write(lat, net, out, utterance="%s/u%d.mfc" % ("r" if c["kind"] == "rescore" else "a", u), lm_name=None, vocab_name="dict",
                             mmf=mmf if align else None)
        assert open(out).read() == open(os.path.join(SETNB, tag, "u%d.%s" % (u, c["latExt"]))).read(), (tag, u)
    want = 1 if (c["nTrans"] > 1 and c["latExt"]) else c["nTrans"]          # "only output 1-best transcription if generating lattices" (HVite.c:797)
    if align:
        alts = native.lattice_nbest_align(lat, net, mmf, want, states=False, models=True)
    else:
        alts = [word_labels(a, net) for a in native.lattice_nbest(lat, net, want)]
    assert alts == c["nbest"]["u%d" % u], (tag, u)
