"""Wall time of data-driven state clustering (TC) on a synthetic single-Gaussian set: the device (Mmf.data_cluster, and the merge loop
alone through capi.cluster_merges) and, where oracle/_ref/HHEd is built, the reference's HHEd on one host core over the same script.

    python tools/data_cluster_bench.py --commands 1 --items 2000 [--dim 39] [--no-hhed]
    python tools/data_cluster_bench.py --commands 120 --items 300

Prints one JSON line; `identical` says whether both wrote the same model set."""
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
from htk_amd import capi, treeclust


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commands", type=int, default=1); ap.add_argument("--items", type=int, default=2000); ap.add_argument("--dim", type=int, default=39)
    ap.add_argument("--threshold", type=float, default=1.2); ap.add_argument("--no-hhed", action="store_true")
    a = ap.parse_args(argv)
    rng = np.random.RandomState(1)
    work = tempfile.mkdtemp()
    names = []
    with open(os.path.join(work, "hmmdefs"), "w") as f:
        f.write("~o <STREAMINFO> 1 %d <VECSIZE> %d <NULLD><USER><DIAGC>\n" % (a.dim, a.dim))
        for c in range(a.commands):
            centre = rng.randn(8, a.dim) * 2
            for i in range(a.items):
                n = "l%d-p%d+r" % (i, c); names.append(n)
                mean = centre[i % 8] + rng.randn(a.dim) * 0.5; var = 0.5 + rng.rand(a.dim)
                f.write('~h "%s"\n<BEGINHMM>\n<NUMSTATES> 3\n<STATE> 2\n<MEAN> %d\n %s\n<VARIANCE> %d\n %s\n<TRANSP> 3\n0 1 0\n0 .5 .5\n0 0 0\n<ENDHMM>\n'
                        % (n, a.dim, " ".join("%e" % x for x in mean), a.dim, " ".join("%e" % x for x in var)))
    open(os.path.join(work, "hmmlist"), "w").write("\n".join(names) + "\n")
    script = "".join('TC %.2f "C%d_" {"*-p%d+*".state[2]}\n' % (a.threshold, c, c) for c in range(a.commands))
    open(os.path.join(work, "tc.hed"), "w").write(script)
    m = capi.Mmf([os.path.join(work, "hmmdefs")], hmm_list=os.path.join(work, "hmmlist"))
    d = capi.state_distances(m, '{"*-p0+*".state[2]}')                       # (also starts the HIP runtime)
    t0 = time.perf_counter(); capi.state_distances(m, '{"*-p0+*".state[2]}'); t_dist = time.perf_counter() - t0
    t0 = time.perf_counter(); capi.cluster_merges(d, 1, a.threshold); t_merge = time.perf_counter() - t0
    t0 = time.perf_counter()
    counts = treeclust.run_script(m, treeclust.parse_script(script))[0]
    t_dev = time.perf_counter() - t0
    m.write(m.packed(), one_file=os.path.join(work, "tied_dev.mmf"))
    res = {"commands": a.commands, "items": a.items, "dim": a.dim, "clusters_first": counts[0], "device_s": round(t_dev, 4),
           "one_command_distances_s": round(t_dist, 4), "one_command_merge_loop_s": round(t_merge, 4)}
    hhed = os.path.join(ROOT, "oracle", "_ref", "HHEd")
    if not a.no_hhed and os.path.exists(hhed):
        t0 = time.perf_counter()
        r = subprocess.run([hhed, "-H", "hmmdefs", "-w", "tied_ref.mmf", "tc.hed", "hmmlist"], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        res["hhed_s"] = round(time.perf_counter() - t0, 3)
        if r.returncode:
            raise SystemExit("HHEd failed:\n" + r.stdout[-2000:])
        res["identical"] = open(os.path.join(work, "tied_ref.mmf"), "rb").read() == open(os.path.join(work, "tied_dev.mmf"), "rb").read()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
