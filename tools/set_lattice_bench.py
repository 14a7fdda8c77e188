"""Word-level alignment to LATTICES of pronunciation alternatives (HVite -a -n 3 -z lat) as a batch -- tools/word_align_bench.py's utterances:
(a) the route before the decoder set's N-best entry points -- per utterance htkamd_net_build_words + a Decoder + run_lattice --
(b) htkamd_net_build_words per utterance, then ONE DecoderSet per 256 utterances and one DecoderSet.run_lattice.
Asserts that every array of every lattice is equal and prints one JSON line.

    python tools/set_lattice_bench.py [--utts 512] [--seed 1] [--toks 3]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from htk_amd import capi  # noqa: E402
from word_align_bench import SRC, synth_utt  # noqa: E402

ROOM = dict(maxNodes=256, maxArcs=1024)      # per utterance: 5-15 words with up to `toks` alternatives each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=512)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--beam", type=float, default=1000.0)
    ap.add_argument("--toks", type=int, default=3)
    a = ap.parse_args()
    mmf = capi.Mmf(files=[os.path.join(SRC, "MMF")], hmm_list=os.path.join(SRC, "hmmlist"))
    pk = mmf.packed()
    model = capi.Model(pk)
    rng = np.random.default_rng(a.seed)
    utts = [synth_utt(pk, rng) for _ in range(a.utts)]
    dic = os.path.join(SRC, "dict")

    def per_utterance(nu):
        out = []
        for words, f in utts[:nu]:
            dec = capi.Decoder(model, capi.Net(None, dic, mmf, words=words))
            out += dec.run_lattice([f], a.toks, genBeam=a.beam, **ROOM)
        return out

    def as_sets(nu, per=256):
        out = []
        for u0 in range(0, nu, per):
            chunk = utts[u0:min(nu, u0 + per)]
            ds = capi.DecoderSet(model, [capi.Net(None, dic, mmf, words=words) for words, _ in chunk])
            out += ds.run_lattice([f for _, f in chunk], list(range(len(chunk))), a.toks, genBeam=a.beam, **ROOM)
        return out

    nw = min(8, a.utts)
    as_sets(nw); per_utterance(nw)                                      # warm-up: the kernels' code objects, the allocator
    t0 = time.perf_counter(); ra = per_utterance(a.utts); ta = time.perf_counter() - t0
    t0 = time.perf_counter(); rb = as_sets(a.utts); tb = time.perf_counter() - t0
    arcs = 0
    for u, (x, y) in enumerate(zip(ra, rb)):
        assert x is not None and y is not None and sorted(x) == sorted(y), u
        for k in x:
            assert np.array_equal(x[k], y[k]), (u, k)
        arcs += len(x["arcStart"])
    wg = int(re.search(r"#define DEC_SET_THREADS (\d+)", open(os.path.join(ROOT, "htk_amd", "csrc", "decode.h")).read()).group(1))
    print(json.dumps(dict(utts=a.utts, frames=int(sum(f.shape[0] for _, f in utts)), toks=a.toks, arcs=arcs, per_utterance_s=round(ta, 4), decoder_set_s=round(tb, 4),
                          speedup=round(ta / tb, 2), per_utterance_utt_per_s=round(a.utts / ta, 1), decoder_set_utt_per_s=round(a.utts / tb, 1), set_size=256, workgroup=wg)))


if __name__ == "__main__":
    main()
