#!/usr/bin/env python3
"""HRest over the synthetic labelled corpus of tools/hinit_bench.py, started from the models htkamd_hinit wrote, measured three ways
(one JSON line):
    one_call_s        every model in one htkamd_hrest call (capi.hrest)
    per_model_s       examples/hrest_model.py::hrest, one model after the other (a batch, an accumulator download and a host update per pass)
    reference_s       the reference's HRest on one core, one process per model (only where oracle/_ref/HRest is built)
Default shape: 48 models x 3 states x 4 components, D = 39, 100 tokens of 12 .. 30 frames per model.

    python tools/hrest_bench.py [--models 48] [--mix 4] [--tokens 100] [--dim 39] [--maxiter 10] [--skip-per-model] [--skip-reference]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tempfile  # noqa: E402

from htk_amd import capi, synth  # noqa: E402
from tools.hinit_bench import corpus, proto_text  # noqa: E402


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
        for sub in ("proto", "start", "lab", "out"):
            os.makedirs(os.path.join(d, sub))
        for n in names:
            open(os.path.join(d, "proto", n), "w").write(proto_text(n, a.dim, a.states, a.mix))
        open(os.path.join(d, "list"), "w").write("\n".join(names) + "\n")
        frame_off = capi.offsets([x.shape[0] for x in files])
        dX = capi.DevArray(np.ascontiguousarray(np.concatenate(files)))
        proto = capi.Mmf(hmm_list=os.path.join(d, "list"), hmm_dir=os.path.join(d, "proto"))
        ppk = proto.packed()
        tok = tokens_from_labels(ppk, proto.logical, frame_off, labels, seg_reject=False)
        started, _ = capi.hinit(ppk, dX.ptr, int(frame_off[-1]), tok, [proto.logical[n] for n in names], capi.hinit_config(max_iter=a.maxiter))
        proto.write(started.get_params(), one_file=None, out_dir=os.path.join(d, "start"), binary=False)     # the models every contender starts from
        mmf = capi.Mmf(hmm_list=os.path.join(d, "list"), hmm_dir=os.path.join(d, "start"))
        pk = mmf.packed()
        cfg = capi.hrest_config(max_iter=a.maxiter)
        models = [mmf.logical[n] for n in names]
        capi.hrest(pk, dX.ptr, int(frame_off[-1]), tok, models[:2], cfg)                 # warm-up: code objects, allocator
        capi.check(capi.lib().htkamd_stream_sync(None), "sync")
        t0 = time.perf_counter()
        model, res = capi.hrest(capi.Model(pk), dX.ptr, int(frame_off[-1]), tok, models, cfg)
        out["one_call_s"] = time.perf_counter() - t0
        out["passes"] = int(sum(r["passes"] for r in res)); out["failed"] = int(sum(r["status"] != 0 for r in res))
        if not a.skip_per_model:
            from examples.hrest_model import hrest
            t0 = time.perf_counter()
            per = 0
            for n in names:
                per += len(hrest(capi, mmf, n, files, labels, max_iter=a.maxiter)[1])
            out["per_model_s"] = time.perf_counter() - t0
            out["per_model_passes"] = per
        ref = os.path.join(ROOT, "oracle", "_ref", "HRest")
        if not a.skip_reference and os.path.exists(ref):
            data = []
            for i, (X, labs) in enumerate(zip(files, labels)):
                data.append(os.path.join(d, "f%d.usr" % i)); synth.write_htk_param(data[-1], X, kind=9)
                open(os.path.join(d, "lab", "f%d.lab" % i), "w").write("".join("%d %d %s\n" % (s, e, n) for n, s, e, _ in labs))
            t0 = time.perf_counter()
            for n in names:
                subprocess.run([ref, "-i", str(a.maxiter), "-L", os.path.join(d, "lab"), "-l", n, "-M", os.path.join(d, "out"), os.path.join(d, "start", n)] + data,
                               check=True, stdout=subprocess.DEVNULL)
            out["reference_s"] = time.perf_counter() - t0
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
