"""One HQuant-sized pool clustered on the device, linear and tree, and the pool coded with the linear table.

    python tools/vq_bench.py [--n 1000000] [--d 39] [--k 256] [--ref-hquant PATH]

Prints one JSON line per run: the call's wall time, the time between its first and last kernel (read-backs included), the rounds of
AllocateVectors (linear) or levels (tree) and the launches.  --ref-hquant: the reference's HQuant built outside the repository; the pool
is written as a parameter file and HQuant timed on one core over it (-n 1 K, Euclidean), for the same clustering.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htk_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=39)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--ref-hquant", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    X = (rng.normal(0, 3, (a.k, a.d))[rng.integers(0, a.k, a.n)] + rng.normal(0, 1, (a.n, a.d))).astype(np.float32)
    dX = capi.DevArray(X)
    lin = None
    for tree in (False, True):
        capi.vq_cluster(dX.ptr, 4096, a.d, 2, tree=tree)                 # (the kernels' first load)
        t0 = time.perf_counter()
        r = capi.vq_cluster(dX.ptr, a.n, a.d, a.k, tree=tree)
        wall = time.perf_counter() - t0
        lin = lin or r
        print(json.dumps(dict(what="vq_cluster", tree=tree, N=a.n, D=a.d, K=a.k, wall_s=round(wall, 4), kernel_s=round(r["kernel_ms"] / 1e3, 4),
                              rounds=r["iterations"], launches=r["launches"], smallest=int(r["size"].min()), largest=int(r["size"].max()))))
    tab = capi.VQ(clusters=[lin], kind=capi.CK_NULLC, magic=9)
    tab.code(dX.ptr, [0, 4096], a.d)
    t0 = time.perf_counter()
    codes = tab.code(dX.ptr, [0, a.n], a.d)
    wall = time.perf_counter() - t0
    print(json.dumps(dict(what="vq_code", N=a.n, D=a.d, K=a.k, wall_s=round(wall, 4), kernel_s=round(tab.kernel_ms / 1e3, 4),
                          agrees_with_cmap=round(float((codes[:, 0] - 1 == lin["cmap"]).mean()), 6))))
    dX.free()
    if a.ref_hquant:
        with tempfile.TemporaryDirectory() as tmp:
            capi.parm_write(os.path.join(tmp, "pool.usr"), X, 100000, 9)
            t0 = time.perf_counter()
            subprocess.check_call([a.ref_hquant, "-n", "1", str(a.k), os.path.join(tmp, "ref.vq"), os.path.join(tmp, "pool.usr")])
            print(json.dumps(dict(what="reference HQuant, one core", N=a.n, D=a.d, K=a.k, wall_s=round(time.perf_counter() - t0, 2))))


if __name__ == "__main__":
    main()
