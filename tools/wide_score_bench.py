#!/usr/bin/env python3
"""Block scoring of wide feature vectors: htkamd_outp_block_mode in HTKAMD_SCORE_EXACT and HTKAMD_SCORE_BF16 (gmm_bf16x.hip).

    python tools/wide_score_bench.py [--states 2000 --mix 16 --frames 4096 --dims 52,78,120 --calls 20 --windows 5 --warmup 3]

One block per vector size (all states x all frames of a synthetic set), both modes alternating window by window.  A window is `calls`
calls between two device events on the stream the library launches on; the figure is the median window's time per call, with the
fastest and slowest beside it.  Also max and rms |bf16 - exact| over the block.  Prints one JSON line.
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
    ap.add_argument("--states", type=int, default=2000)
    ap.add_argument("--mix", type=int, default=16)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--dims", default="52,78,120")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("wide_score_bench: no GPU")
    capi.check(capi.lib().htkamd_set_device(0), "set_device")
    torch.cuda.set_device(0)
    null = torch.cuda.default_stream()               # the library launches on the null stream (stream argument NULL)
    NS, T = a.states, a.frames
    res = {"states": NS, "mix": a.mix, "frames": T, "calls": a.calls, "windows": a.windows, "sizes": []}
    for D in [int(d) for d in a.dims.split(",")]:
        nu = max(1, T // 512)
        s = synth.generate_fast(NS, a.mix, (NS + 2) // 3, nu, (T + nu - 1) // nu, 7, D=D)
        X = np.concatenate(s.feats)[:T]
        model = capi.Model(s.packed())
        dX, dS, dO = capi.DevArray(X), capi.DevArray(np.arange(NS, dtype=np.int32)), capi.DevArray(nbytes=4 * T * NS)

        def call(mode):
            capi.check(capi.lib().htkamd_outp_block_mode(model.h, dX.ptr, T, dS.ptr, NS, dO.ptr, T, mode, None), "outp_block")

        out, ms = {}, {capi.SCORE_EXACT: [], capi.SCORE_BF16: []}
        for mode in ms:
            for _ in range(a.warmup):
                call(mode)
            out[mode] = dO.to_host(np.float32, (NS, T)).astype(np.float64)
        for _ in range(a.windows):
            for mode in ms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(null)
                for _ in range(a.calls):
                    call(mode)
                e1.record(null)
                e1.synchronize()
                ms[mode].append(e0.elapsed_time(e1) / a.calls)
        diff = out[capi.SCORE_BF16] - out[capi.SCORE_EXACT]
        ex, bf = sorted(ms[capi.SCORE_EXACT]), sorted(ms[capi.SCORE_BF16])
        res["sizes"].append({"D": D, "exact_ms": round(float(np.median(ex)), 4), "exact_ms_range": [round(ex[0], 4), round(ex[-1], 4)],
                             "bf16_ms": round(float(np.median(bf)), 4), "bf16_ms_range": [round(bf[0], 4), round(bf[-1], 4)],
                             "exact_over_bf16": round(float(np.median(ex) / np.median(bf)), 3),
                             "max_abs_diff": float(np.abs(diff).max()), "rms_diff": float(np.sqrt((diff ** 2).mean()))})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
