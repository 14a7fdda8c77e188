#!/usr/bin/env python3
"""Mixture statistics (UpMixParms) of a pass over sets the state-bucketed kernel of D = 13 / 26 / 39 with <= 16 components does not take:
other vector sizes (k_mixstate_x with one or two wavefronts per workgroup) and larger mixtures (several component tiles).

    python tools/wide_mix_bench.py [--states 5000 --utts 1250 --frames 500 --sizes 36x16,52x16,78x16,120x16,39x32 --passes 10 --windows 5 --warmup 3]

One synthetic shard per size (the default is the size of bench.py's shard), one pass in the tolerance class (bf16 x 3 scores, fp32-transcendental LAdd) per call of
ForwardBackward.execute; the figure is the pass's mixture-statistics interval (kernel_times()[3]: the stream events around its
launches).  A window is the mean over `passes` passes; the median window is reported with the fastest and slowest beside it.
Only the public binding is used, so the same script measures any earlier build of the library from that build's tree.
Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from htk_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=5000)
    ap.add_argument("--utts", type=int, default=1250)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--sizes", default="36x16,52x16,78x16,120x16,39x32", help="DxM, comma separated")
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("wide_mix_bench: no GPU")
    capi.check(capi.lib().htkamd_set_device(0), "set_device")
    NS = a.states
    res = {"states": NS, "utts": a.utts, "frames": a.frames, "passes": a.passes, "windows": a.windows, "sizes": []}
    cfg = capi.fb_config(scoreMode=capi.SCORE_BF16 | capi.SCORE_FASTLADD)
    for D, M in [tuple(int(v) for v in sz.split("x")) for sz in a.sizes.split(",")]:
        s = synth.generate_fast(NS, M, (NS + 2) // 3, a.utts, a.frames, 7, D=D)
        model = capi.Model(s.packed())
        X = np.concatenate(s.feats).astype(np.float32)
        frameOff = np.concatenate([[0], np.cumsum([len(x) for x in s.feats])]).astype(np.int32)
        labOff = np.concatenate([[0], np.cumsum([len(q) for q in s.seqs])]).astype(np.int32)
        labs = np.concatenate(s.seqs).astype(np.int32)
        dX = capi.DevArray(X)
        fb, acc = capi.ForwardBackward(model), capi.Accs(model)
        fb.prepare(dX.ptr.value, frameOff, labOff, labs)

        def one_pass():
            acc.zero()
            fb.execute(cfg, acc)
            return fb.kernel_times()[3] * 1e3      # (waits for the pass's last event)

        for _ in range(a.warmup):
            one_pass()
        assert (fb.results()[1] == 1).all()
        win = sorted(float(np.mean([one_pass() for _ in range(a.passes)])) for _ in range(a.windows))
        res["sizes"].append({"D": D, "M": M, "total_frames": int(len(X)), "mix_counts": list(fb.mix_counts()),
                             "mix_ms": round(float(np.median(win)), 4), "mix_ms_range": [round(win[0], 4), round(win[-1], 4)]})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
