#!/usr/bin/env python3
"""Timing of side-based normalisation on the device: htkamd_side_stats and htkamd_parm_normalise on a synthetic table.

    python tools/cepsnorm_bench.py [--utts 2000 --frames 500 --cols 39 --sides 200 --calls 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/cepsnorm_bench.py ...      # kernel times, in a run of its own

Prints one JSON line: the shape, the bytes each kernel has to move (from the shape: the table read once by k_side_partial; read and
written once, plus the 4-byte side of every row, by k_side_normalise) and the time of a whole call -- a host clock around the
synchronising call, scratch allocation and table uploads included.  A kernel's bytes per second = its bytes here over its time in the trace.
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
    ap.add_argument("--sides", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    capi.check(capi.lib().htkamd_set_device(0), "set_device")
    U, T, D, S = a.utts, a.frames, a.cols, a.sides
    rng = np.random.default_rng(1)
    X = rng.normal(0, 3, (U * T, D)).astype(np.float32)
    frameOff = (np.arange(U + 1) * T).astype(np.int32)
    uttSide = (np.arange(U) % S).astype(np.int32)
    mean = rng.normal(0, 1e-3, (S, D)).astype(np.float32)
    scale = np.ones((S, D), np.float32)
    dX = capi.DevArray(X)
    for _ in range(a.warmup):
        capi.side_stats(dX.ptr, frameOff, uttSide, S, D, D)
        capi.parm_normalise(dX.ptr, frameOff, uttSide, S, D, mean=mean, scale=scale)
    t0 = time.perf_counter()
    for _ in range(a.calls):
        capi.side_stats(dX.ptr, frameOff, uttSide, S, D, D)
    t1 = time.perf_counter()
    for _ in range(a.calls):
        capi.parm_normalise(dX.ptr, frameOff, uttSide, S, D, mean=mean, scale=scale)
    t2 = time.perf_counter()
    table = U * T * D * 4
    bytes_ = {"k_side_partial": table + U * 2 * D * 8, "k_side_merge": U * 2 * D * 8 + S * 2 * D * 8,
              "k_row_side": U * T * 4, "k_side_normalise": 2 * table + U * T * 4}
    stats_ms, norm_ms = (t1 - t0) / a.calls * 1e3, (t2 - t1) / a.calls * 1e3
    print(json.dumps({"utts": U, "frames": T, "cols": D, "sides": S, "table_MB": table / 1e6, "kernel_bytes": bytes_,
                      "side_stats_call_ms": stats_ms, "parm_normalise_call_ms": norm_ms,
                      "side_stats_call_GBps": bytes_["k_side_partial"] / stats_ms / 1e6,
                      "parm_normalise_call_GBps": bytes_["k_side_normalise"] / norm_ms / 1e6}))


if __name__ == "__main__":
    main()
