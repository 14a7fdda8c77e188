#!/usr/bin/env python3
"""Timing of the global linear input transform on the device: htkamd_parm_xform on the synthetic table of tools/cepsnorm_bench.py, with
htkamd_parm_normalise (k_side_normalise, which reads and writes the same table once) timed beside it in the same run as the yardstick.

    python tools/xform_bench.py [--utts 2000 --frames 500 --cols 39 --rows 39 20 --sides 200 --calls 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/xform_bench.py ...      # kernel times, in a run of its own

Prints one JSON line: the shape, the bytes each kernel has to move (from the shape: k_side_normalise reads and writes the table once plus
the 4-byte side of every row; k_parm_xform reads the table once and writes rows x mrows floats) and the time of a whole call -- a host
clock around the call and the synchronisation behind it.  A kernel's bytes per second = its bytes here over its time in the trace.  The
transform is timed out of place (--rows below --cols cannot be in place) for every --rows value.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from htk_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--cols", type=int, default=39)
    ap.add_argument("--rows", type=int, nargs="+", default=[39, 20])
    ap.add_argument("--sides", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    capi.check(capi.lib().htkamd_set_device(0), "set_device")
    U, T, D, S = a.utts, a.frames, a.cols, a.sides
    F = U * T
    rng = np.random.default_rng(1)
    X = rng.normal(0, 3, (F, D)).astype(np.float32)
    frameOff = (np.arange(U + 1) * T).astype(np.int32)
    uttSide = (np.arange(U) % S).astype(np.int32)
    mean = rng.normal(0, 1e-3, (S, D)).astype(np.float32)
    scale = np.ones((S, D), np.float32)
    dX = capi.DevArray(X)
    del X
    sync = lambda: capi.check(capi.lib().htkamd_stream_sync(None), "stream_sync")
    table = F * D * 4
    out = {"utts": U, "frames": T, "cols": D, "sides": S, "table_MB": table / 1e6, "kernel_bytes": {"k_side_normalise": 2 * table + F * 4}}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        return (time.perf_counter() - t0) / a.calls * 1e3

    out["parm_normalise_call_ms"] = timed(lambda: capi.parm_normalise(dX.ptr, frameOff, uttSide, S, D, mean=mean, scale=scale))
    out["parm_normalise_call_GBps"] = out["kernel_bytes"]["k_side_normalise"] / out["parm_normalise_call_ms"] / 1e6
    for R in a.rows:
        dM = capi.DevArray((rng.normal(0, 1, (R, D)) / np.sqrt(D)).astype(np.float32))
        dOut = capi.DevArray(nbytes=4 * F * R)

        def xform():
            capi.parm_xform(dX.ptr, D, dOut.ptr, R, F, dM.ptr, R, D)
            sync()
        key = "k_parm_xform_%dx%d" % (R, D)
        out["kernel_bytes"][key] = table + F * R * 4
        out["parm_xform_%dx%d_call_ms" % (R, D)] = ms = timed(xform)
        out["parm_xform_%dx%d_call_GBps" % (R, D)] = out["kernel_bytes"][key] / ms / 1e6
        out["parm_xform_%dx%d_call_GFLOPs" % (R, D)] = 2.0 * F * R * D / ms / 1e6
        del dOut
    print(json.dumps(out))


if __name__ == "__main__":
    main()
