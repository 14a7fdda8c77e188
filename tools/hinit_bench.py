#!/usr/bin/env python3
"""HInit over a synthetic labelled corpus, measured three ways (one JSON line):
    one_call_s        every model in one htkamd_hinit call (capi.hinit)
    per_model_s       examples/hinit_model.py::hinit, one model after the other (host loops, a device round trip per pass)
    reference_s       the reference's HInit on one core, one process per model (only where oracle/_ref/HInit is built)
Default shape: 48 models x 3 states x 4 components, D = 39, 100 tokens of 12 .. 30 frames per model.

    python tools/hinit_bench.py [--models 48] [--mix 4] [--tokens 100] [--dim 39] [--maxiter 10] [--skip-per-model] [--skip-reference]
"""
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
from htk_amd import capi, synth  # noqa: E402


def proto_text(name, D, ne, M):
    N = ne + 2
    out = ["~o <VecSize> %d <USER> <StreamInfo> 1 %d" % (D, D), '~h "%s"' % name, "<BeginHMM>", "<NumStates> %d" % N]
    for s in range(2, N):
        out.append("<State> %d <NumMixes> %d" % (s, M))
        for m in range(M):
            out += ["<Mixture> %d %.4f" % (m + 1, 1.0 / M), "<Mean> %d" % D, " ".join(["0.0"] * D), "<Variance> %d" % D, " ".join(["1.0"] * D)]
    out.append("<TransP> %d" % N)
    for i in range(N):
        row = [0.0] * N
        if i == 0:
            row[1] = 1.0
        elif i < N - 1:
            row[i], row[i + 1] = 0.6, 0.4
        out.append(" ".join("%.3e" % x for x in row))
    return "\n".join(out + ["<EndHMM>"]) + "\n"


def corpus(names, D, ne, M, tokens, seed=5):
    """one file per 'utterance' of len(names) tokens, every model once per file; labels as HInit reads them"""
    r = np.random.RandomState(seed)
    centre = {n: 3.0 * r.randn(ne, M, D) for n in names}
    files, labels = [], []
    for _ in range(tokens):
        rows, labs, t = [], [], 0
        for n in names:
            L = int(r.randint(12, 31))
            st = (np.arange(L) * ne) // L
            x = centre[n][st, r.randint(0, M, L)] + r.randn(L, D)
            rows.append(x); labs.append((n, t * 100000, (t + L - 1) * 100000, 0.0)); t += L
        files.append(np.concatenate(rows).astype(np.float32)); labels.append(labs)
    return files, labels


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", type=int, default=48); ap.add_argument("--states", type=int, default=3); ap.add_argument("--mix", type=int, default=4)
    ap.add_argument("--dim", type=int, default=39); ap.add_argument("--tokens", type=int, default=100); ap.add_argument("--maxiter", type=int, default=10)
    ap.add_argument("--skip-per-model", action="store_true"); ap.add_argument("--skip-reference", action="store_true")
    a = ap.parse_args(argv)
    from examples.hinit_set import tokens_from_labels
    names = ["m%02d" % k for k in range(a.models)]
    files, labels = corpus(names, a.dim, a.states, a.mix, a.tokens)
    out = dict(models=a.models, states=a.states, mix=a.mix, dim=a.dim, tokens=a.models * a.tokens, frames=int(sum(x.shape[0] for x in files)), maxiter=a.maxiter)
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "proto")); os.makedirs(os.path.join(d, "lab")); os.makedirs(os.path.join(d, "out"))
        for n in names:
            open(os.path.join(d, "proto", n), "w").write(proto_text(n, a.dim, a.states, a.mix))
        open(os.path.join(d, "list"), "w").write("\n".join(names) + "\n")
        mmf = capi.Mmf(hmm_list=os.path.join(d, "list"), hmm_dir=os.path.join(d, "proto"))
        pk = mmf.packed()
        frame_off = capi.offsets([x.shape[0] for x in files])
        dX = capi.DevArray(np.ascontiguousarray(np.concatenate(files)))
        tok = tokens_from_labels(pk, mmf.logical, frame_off, labels)
        cfg = capi.hinit_config(max_iter=a.maxiter)
        models = [mmf.logical[n] for n in names]
        capi.hinit(pk, dX.ptr, int(frame_off[-1]), tok, models[:2], cfg)                 # warm-up: code objects, allocator
        capi.check(capi.lib().htkamd_stream_sync(None), "sync")
        t0 = time.perf_counter()
        model, res = capi.hinit(capi.Model(pk), dX.ptr, int(frame_off[-1]), tok, models, cfg)
        out["one_call_s"] = time.perf_counter() - t0
        out["passes"] = int(sum(r["passes"] for r in res)); out["failed"] = int(sum(r["status"] != 0 for r in res))
        if not a.skip_per_model:
            from examples.hinit_model import hinit
            t0 = time.perf_counter()
            for n in names:
                hinit(capi, mmf, n, files, labels, max_iter=a.maxiter)
            out["per_model_s"] = time.perf_counter() - t0
        ref = os.path.join(ROOT, "oracle", "_ref", "HInit")
        if not a.skip_reference and os.path.exists(ref):
            data = []
            for i, (X, labs) in enumerate(zip(files, labels)):
                data.append(os.path.join(d, "f%d.usr" % i)); synth.write_htk_param(data[-1], X, kind=9)
                open(os.path.join(d, "lab", "f%d.lab" % i), "w").write("".join("%d %d %s\n" % (s, e, n) for n, s, e, _ in labs))
            t0 = time.perf_counter()
            for n in names:
                subprocess.run([ref, "-i", str(a.maxiter), "-L", os.path.join(d, "lab"), "-l", n, "-o", n, "-M", os.path.join(d, "out"), os.path.join(d, "proto", n)] + data,
                               check=True, stdout=subprocess.DEVNULL)
            out["reference_s"] = time.perf_counter() - t0
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
