#!/usr/bin/env python3
"""Full-covariance statistics of a frame table (htkamd_compv_full, csrc/compv_full.hip) at the size of a training set.

    python tools/compv_full_bench.py [--frames 1000000 --calls 5 --windows 5 --warmup 2 --peak-tflops 78.6 --no-reference]

Three cases over seeded random tables: frames x 39 as one class, frames x 120 as one class, frames x 39 as 4 096 label segments over
48 classes.  Per case: kernel_ms, the event interval around the call's two kernels (htkamd_compv_full_last_kernel_ms), and call_ms, the
host clock around the whole call (it ends in a stream synchronise: chunk list, uploads, scratch allocation, kernels, copy back).  A
window is the mean over `calls` calls; the median window is reported with the fastest and slowest beside it.  mfma_share is the
arithmetic the matrix instructions carry out (lower-triangle tiles of the padded augmented row, every started K step of 4 frames)
over kernel_ms, as a share of the fp64 matrix peak (--peak-tflops: the vendor's published figure for the MI355X); useful_tflops
counts only the (D+1)(D+2)/2 products per frame a caller asked for.  Beside them: htkamd_compv on the same 39-column table (mean and
diagonal variance: 1/20 of the arithmetic, so a floor and not a bar; call time, it has no event interval of its own) and, where
oracle/_ref/HCompV exists, the reference's one-core time on the same 39-column table written as one parameter file, for a FULLC
prototype.  Prints one JSON line.
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from htk_amd import capi  # noqa: E402


def windows(fn, calls, n_windows):
    """Per figure fn returns: (median, fastest, slowest) of the windows' means."""
    w = np.array([np.mean([fn() for _ in range(calls)], axis=0) for _ in range(n_windows)])
    return [(round(float(np.median(c)), 4), round(float(c.min()), 4), round(float(c.max()), 4)) for c in w.T]


def mfma_flops(D, segs, chunk):
    nt = (D + 1 + 15) // 16
    ksteps = sum(((n % chunk) + 3) // 4 + (n // chunk) * (chunk // 4) for _, n, _ in segs)
    return nt * (nt + 1) // 2 * ksteps * 2 * 16 * 16 * 4


def reference_seconds(X, tmp):
    D = X.shape[1]
    capi.parm_write(os.path.join(tmp, "all.mfc"), X, 100000, 9)      # USER vectors
    rows = "\n".join("".join(" %.1f" % (1.0 if j == i else 0.0) for j in range(i, D)) for i in range(D))
    with open(os.path.join(tmp, "proto"), "w") as f:
        f.write("~o <VecSize> %d <USER>\n~h \"proto\"\n<BeginHMM>\n<NumStates> 3\n<State> 2\n<Mean> %d\n%s\n<InvCovar> %d\n%s\n"
                "<TransP> 3\n 0.0 1.0 0.0\n 0.0 0.6 0.4\n 0.0 0.0 0.0\n<EndHMM>\n" % (D, D, " 0.0" * D, D, rows))
    os.makedirs(os.path.join(tmp, "out"))
    t0 = time.perf_counter()
    subprocess.check_call([os.path.join(ROOT, "oracle", "_ref", "HCompV"), "-m", "-M", "out", "proto", "all.mfc"], cwd=tmp)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()
    if capi.lib().htkamd_device_count() < 1:
        sys.exit("compv_full_bench: no GPU")
    capi.check(capi.lib().htkamd_set_device(0), "set_device")
    F, chunk = a.frames, capi.compv_full_chunk()
    rng = np.random.default_rng(5)
    cuts = np.sort(rng.choice(np.arange(1, F), 4095, replace=False))
    bounds = np.concatenate([[0], cuts, [F]])
    labelled = [(int(b0), int(b1 - b0), int(k)) for b0, b1, k in zip(bounds[:-1], bounds[1:], rng.integers(0, 48, 4096))]
    res = {"frames": F, "chunk": chunk, "calls": a.calls, "windows": a.windows, "peak_tflops": a.peak_tflops, "cases": []}
    X39 = None
    for name, D, segs, K in (("39_one_class", 39, None, 1), ("120_one_class", 120, None, 1), ("39_4096_segments_48_classes", 39, labelled, 48)):
        X = (rng.standard_normal((F, D), dtype=np.float32) * 8.0 + 10.0)
        dX = capi.DevArray(X)

        def one():
            t0 = time.perf_counter()
            capi.compv_full(dX.ptr, F, D, segs=segs, nClass=K)
            return (time.perf_counter() - t0) * 1e3, capi.compv_full_kernel_ms()

        for _ in range(a.warmup):
            one()
        call, kern = windows(one, a.calls, a.windows)
        issued = mfma_flops(D, segs or [(0, F, 0)], chunk)
        case = {"case": name, "D": D, "kernel_ms": kern[0], "kernel_ms_range": list(kern[1:]), "call_ms": call[0], "call_ms_range": list(call[1:]),
                "mfma_tflops": round(issued / kern[0] * 1e-9, 2), "mfma_share": round(issued / kern[0] * 1e-9 / a.peak_tflops, 4),
                "useful_tflops": round(F * (D + 1) * (D + 2) / kern[0] * 1e-9, 2)}
        if name == "39_one_class":
            X39 = X

            def diag():
                t0 = time.perf_counter()
                capi.compv(dX.ptr, F, D)
                return ((time.perf_counter() - t0) * 1e3,)

            for _ in range(a.warmup):
                diag()
            d = windows(diag, a.calls, a.windows)[0]
            case["compv_diag_call_ms"], case["compv_diag_call_ms_range"] = d[0], list(d[1:])
        res["cases"].append(case)
        dX.free()
    if not a.no_reference and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "HCompV")):
        with tempfile.TemporaryDirectory() as tmp:
            res["reference_hcompv_fullc_39_one_core_s"] = round(reference_seconds(X39, tmp), 2)
    else:
        res["reference_hcompv_fullc_39_one_core_s"] = None      # not measured
    print(json.dumps(res))


if __name__ == "__main__":
    main()
