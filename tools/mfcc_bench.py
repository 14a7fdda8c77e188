"""Throughput of the device front end at BASELINE config[4]: 16 kHz mono PCM, 25 ms / 10 ms, 26 channels, 12 cepstra,
MFCC_0_D_A, 3-second utterances (298 frames).  Waveforms resident on the device; time = htkamd_mfcc_compute only.
(The CPU side of the comparison -- the reference's HCopy on one core -- is measured separately; tools never touch oracle/.)
--kind K codes TARGETKIND K instead (PLP_0_D_A, FBANK_E_D_A, MELSPEC, ...: htkamd_frontend_compute, 40 channels for FBANK / MELSPEC);
the default run is the MFCC_0_D_A one through htkamd_mfcc_compute.
--warps K times the VTLN warp grid instead (K factors from 0.88 to 1.12, cut-offs 300 / 3400): (a) one htkamd_frontend_compute_grid call,
(b) K htkamd_frontend_compute_warped calls, each with one warp for all utterances, (c) a plain un-warped htkamd_frontend_compute call;
the best of 5 runs each, in ms.
Run on the GPU box: python tools/mfcc_bench.py [nUtt] [--kind K] [--warps K]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from htk_amd import capi  # noqa: E402


def bench_warps(kind, K, waves, n, nU):
    fb = kind.upper().split("_")[0] in ("FBANK", "MELSPEC")
    cfg = capi.frontend_config(kind, numChans=40 if fb else 26, usePower=kind.upper().startswith("PLP"))
    L = capi.lib()
    fe = capi.FrontEnd(cfg, warps=[(float(a), 300.0, 3400.0) for a in np.linspace(0.88, 1.12, K)])
    plain = capi.FrontEnd(cfg)
    sampOff = capi.offsets([len(w) for w in waves])
    allw = np.concatenate(waves)
    frames = L.htkamd_frontend_num_frames(C.byref(cfg), C.c_int(n)) * nU
    dW = capi.DevArray(allw)
    dO = capi.DevArray(nbytes=4 * frames * fe.cols * K)
    frameOff = np.zeros(nU + 1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    idx = [np.full(nU, w, np.int32) for w in range(K)]

    def grid():
        capi.check(L.htkamd_frontend_compute_grid(fe.h, dW.ptr, p(sampOff), C.c_int(nU), p(frameOff), dO.ptr, None), "compute_grid")

    def singles():
        for w in range(K):
            capi.check(L.htkamd_frontend_compute_warped(fe.h, dW.ptr, p(sampOff), C.c_int(nU), p(idx[w]), p(frameOff), dO.ptr, None), "compute_warped")

    def unwarped():
        capi.check(L.htkamd_frontend_compute(plain.h, dW.ptr, p(sampOff), C.c_int(nU), p(frameOff), dO.ptr, None), "compute")

    out = {}
    for name, fn in (("grid", grid), ("singles", singles), ("plain", unwarped)):
        ts = []
        for rep in range(6):                   # the first run warms up (buffers of the handle)
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = ts[1:]
    print("%s, %d utterances, %d frames, %d warps:" % (kind, nU, frames, K))
    print("  (a) one grid call                     best %.2f ms  (runs %s)" % (min(out["grid"]), " ".join("%.2f" % t for t in out["grid"])))
    print("  (b) %2d constant-warp calls            best %.2f ms  (runs %s)" % (K, min(out["singles"]), " ".join("%.2f" % t for t in out["singles"])))
    print("  (c) one un-warped call                best %.2f ms  (runs %s); x %d = %.2f ms"
          % (min(out["plain"]), " ".join("%.2f" % t for t in out["plain"]), K, K * min(out["plain"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("nUtt", nargs="?", type=int, default=2000)
    ap.add_argument("--kind", default=None)
    ap.add_argument("--warps", type=int, default=0)
    args = ap.parse_args()
    nU = args.nUtt
    rng = np.random.default_rng(7)
    n = 48000
    t = np.arange(n) / 16000.0
    base = (3000 * np.sin(2 * np.pi * 440 * t) + 2000 * np.sin(2 * np.pi * 1800 * t)).astype(np.float32)
    waves = [(base + rng.normal(0, 500, n)).astype(np.int16) for _ in range(8)]
    waves = [waves[i % 8] for i in range(nU)]
    if args.warps:
        return bench_warps(args.kind or "MFCC_0_D_A", args.warps, waves, n, nU)
    if args.kind is None:
        cfg = capi.mfcc_config("MFCC_0_D_A")
        fe, num_frames, compute = capi.Mfcc(cfg), capi.lib().htkamd_mfcc_num_frames, capi.lib().htkamd_mfcc_compute
    else:
        fb = args.kind.upper().split("_")[0] in ("FBANK", "MELSPEC")
        cfg = capi.frontend_config(args.kind, numChans=40 if fb else 26, usePower=args.kind.upper().startswith("PLP"))
        fe, num_frames, compute = capi.FrontEnd(cfg), capi.lib().htkamd_frontend_num_frames, capi.lib().htkamd_frontend_compute
    sampOff = capi.offsets([len(w) for w in waves])
    allw = np.concatenate(waves)
    frames = num_frames(C.byref(cfg), C.c_int(n)) * nU
    dW = capi.DevArray(allw)
    dO = capi.DevArray(nbytes=4 * frames * fe.cols)
    frameOff = np.zeros(nU + 1, np.int32)
    for rep in range(3):
        t0 = time.perf_counter()
        capi.check(compute(fe.h, dW.ptr, allw.ctypes.data_as(C.c_void_p) and sampOff.ctypes.data_as(C.c_void_p), C.c_int(nU),
                           frameOff.ctypes.data_as(C.c_void_p), dO.ptr, None), "compute")
        dt = time.perf_counter() - t0
        print(("%s " % args.kind if args.kind else "") + "GPU run %d: %d utterances, %d frames in %.2f ms = %.2f M frames/s, %.2f GB/s of PCM, %.0f x real time"
              % (rep, nU, frames, dt * 1e3, frames / dt / 1e6, allw.nbytes / dt / 1e9, nU * 3.0 / dt))


if __name__ == "__main__":
    main()
