"""Word-level forced alignment (HVite -a from word transcriptions, dictionary with pronunciation variants) as a batch:
(a) the route before the decoder set -- per utterance htkamd_net_build_words + htkamd_decoder_create + htkamd_decoder_run + destroy, what
    tools/hvite.c did for every file --
(b) htkamd_net_build_words per utterance, then ONE htkamd_decoder_set per 256 utterances and one htkamd_decoder_set_run.
Both through the C ABI (ctypes), features on the device once.  Asserts that the results are equal and prints one JSON line.

    python tools/word_align_bench.py [--utts 512] [--seed 1]
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from htk_amd import capi  # noqa: E402

SRC = os.path.join(ROOT, "tests", "golden", "decode", "bigram")
PRONS = {"AB": [[0, 1], [0, 2]], "CD": [[3, 4, 5]], "E": [[6]], "F": [[7]], "G": [[8, 9]], "H": [[10]], "I": [[11]]}      # the case's dictionary
MAXW = 64


def synth_utt(pk, rng):
    """5-15 words, 200-600 frames drawn from the states of one pronunciation of each."""
    words = [list(PRONS)[k] for k in rng.integers(0, len(PRONS), size=int(rng.integers(5, 16)))]
    phones = [ph for w in words for ph in PRONS[w][int(rng.integers(0, len(PRONS[w])))]]
    states = [pk["hmmState"][j] for ph in phones for j in range(pk["hmmStateOff"][ph], pk["hmmStateOff"][ph + 1])]
    T = int(rng.integers(200, 601))
    dur = np.full(len(states), T // len(states)); dur[:T - dur.sum()] += 1
    fr = []
    for st, n in zip(states, dur):
        g = pk["compGauss"][rng.integers(pk["stateCompOff"][st], pk["stateCompOff"][st + 1])]
        fr.append(pk["mean"][g] + np.sqrt(pk["var"][g]) * rng.normal(size=(int(n), pk["vecSize"])))
    return words, np.concatenate(fr).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=512)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--beam", type=float, default=250.0)
    a = ap.parse_args()
    L = capi.lib()
    mmf = capi.Mmf(files=[os.path.join(SRC, "MMF")], hmm_list=os.path.join(SRC, "hmmlist"))
    pk = mmf.packed()
    model = capi.Model(pk)
    rng = np.random.default_rng(a.seed)
    utts = [synth_utt(pk, rng) for _ in range(a.utts)]
    X = np.concatenate([f for _, f in utts])
    frameOff = capi.offsets([f.shape[0] for _, f in utts])
    dX = capi.DevArray(X)
    D = X.shape[1]
    dictp = os.path.join(SRC, "dict").encode()
    cfg = capi.DecodeConfig(a.beam, 1.0e10, 1.0, 0.0, 1.0, 0, 0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)

    def build_net(words):
        h = C.c_void_p()
        arr = (C.c_char_p * len(words))(*[w.encode() for w in words])
        capi.check(L.htkamd_net_build_words(arr, C.c_int(len(words)), None, dictp, mmf.h, C.byref(h)), "net_build_words")
        return h

    def outputs(n):
        return dict(nW=np.zeros(n, np.int32), pron=np.zeros((n, MAXW), np.int32), st=np.zeros((n, MAXW), np.int32), en=np.zeros((n, MAXW), np.int32),
                    sc=np.zeros((n, MAXW), np.float32), lm=np.zeros((n, MAXW), np.float32), tot=np.zeros(n, np.float64))

    def per_utterance(nu):
        o = outputs(nu)
        fo = np.zeros(2, np.int32)
        for u, (words, f) in enumerate(utts[:nu]):
            net = build_net(words)
            dec = C.c_void_p()
            capi.check(L.htkamd_decoder_create(model.h, L.htkamd_net_get(net), C.c_float(1.0), C.byref(dec)), "decoder_create")
            fo[1] = f.shape[0]
            capi.check(L.htkamd_decoder_run(dec, C.byref(cfg), C.c_void_p(dX.ptr.value + 4 * D * int(frameOff[u])), p(fo), C.c_int(1), C.c_int(MAXW),
                                            p(o["nW"][u:]), p(o["pron"][u]), p(o["st"][u]), p(o["en"][u]), p(o["sc"][u]), p(o["lm"][u]), p(o["tot"][u:]), None), "decoder_run")
            L.htkamd_decoder_destroy(dec); L.htkamd_net_destroy(net)
        return o

    def as_sets(nu, per=256):
        o = outputs(nu)
        for u0 in range(0, nu, per):
            u1 = min(nu, u0 + per)
            nets = [build_net(words) for words, _ in utts[u0:u1]]
            arr = (C.POINTER(capi.NetDesc) * len(nets))(*[L.htkamd_net_get(h) for h in nets])
            ds = C.c_void_p()
            capi.check(L.htkamd_decoder_set_create(model.h, arr, C.c_int(len(nets)), C.c_float(1.0), C.byref(ds)), "decoder_set_create")
            fo = np.ascontiguousarray(frameOff[u0:u1 + 1] - frameOff[u0])
            net_of = np.arange(u1 - u0, dtype=np.int32)
            out = capi.DecodeOut(p(o["nW"][u0:]), p(o["pron"][u0]), p(o["st"][u0]), p(o["en"][u0]), p(o["sc"][u0]), p(o["lm"][u0]), None, None, p(o["tot"][u0:]), None)
            capi.check(L.htkamd_decoder_set_run(ds, C.byref(cfg), C.c_void_p(dX.ptr.value + 4 * D * int(frameOff[u0])), p(fo), p(net_of), C.c_int(u1 - u0), C.c_int(MAXW),
                                                C.byref(out), None), "decoder_set_run")
            L.htkamd_decoder_set_destroy(ds)
            for h in nets:
                L.htkamd_net_destroy(h)
        return o

    nw = min(8, a.utts)
    as_sets(nw); per_utterance(nw)                                      # warm-up: the kernels' code objects, the allocator
    t0 = time.perf_counter(); ra = per_utterance(a.utts); ta = time.perf_counter() - t0
    t0 = time.perf_counter(); rb = as_sets(a.utts); tb = time.perf_counter() - t0
    assert np.array_equal(ra["nW"], rb["nW"]) and np.array_equal(ra["tot"], rb["tot"]) and (ra["nW"] > 0).all()
    for u in range(a.utts):
        n = int(ra["nW"][u])
        for k in ("pron", "st", "en", "sc", "lm"):
            assert np.array_equal(ra[k][u, :n], rb[k][u, :n]), (u, k)
    wg = int(re.search(r"#define DEC_SET_THREADS (\d+)", open(os.path.join(ROOT, "htk_amd", "csrc", "decode.h")).read()).group(1))
    print(json.dumps(dict(utts=a.utts, frames=int(frameOff[-1]), per_utterance_s=round(ta, 4), decoder_set_s=round(tb, 4), speedup=round(ta / tb, 2),
                          per_utterance_utt_per_s=round(a.utts / ta, 1), decoder_set_utt_per_s=round(a.utts / tb, 1), set_size=256, workgroup=wg)))


if __name__ == "__main__":
    main()
