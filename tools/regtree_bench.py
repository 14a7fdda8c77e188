"""Wall time of a regression class tree (HHEd's RC) over a synthetic set: the library call (Mmf.regtree, the splits on the device) and,
where oracle/_ref/HHEd is built, the reference's HHEd on one host core over the same files.

    python tools/regtree_bench.py [--states 5000] [--mixes 16] [--dim 39] [--terminals 32] [--no-hhed]

HHEd's figure is its run with `LS stats` + `RC N` less its run with `LS stats` + `RC 1` (loading the set, the scan and the root's figures:
what is left is the splitting, so the figure flatters HHEd a little).  Prints one JSON
line: call_s the library call, kernel_s the device time of its kernels and kernel_share their share of the call -- the rest is host work
(the scan, the AccSum rows, the upload, one synchronisation per split); `identical` says whether both wrote the same two files."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from htk_amd import capi, regtree_sets as rs      # noqa: E402

HHED = os.path.join(ROOT, "oracle", "_ref", "HHEd")


def run_hhed(work, script, out):
    subprocess.run([HHED, "-H", "hmmdefs", "-M", out, script, "hmmlist"], cwd=work, check=True, stdout=subprocess.DEVNULL)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--states", type=int, default=5000); ap.add_argument("--mixes", type=int, default=16); ap.add_argument("--dim", type=int, default=39)
    ap.add_argument("--terminals", type=int, default=32); ap.add_argument("--no-hhed", action="store_true")
    a = ap.parse_args(argv)
    work = tempfile.mkdtemp()
    emit = 5
    rs.write_set(work, rs.names_for(max(a.states // emit, 1)), emit, a.mixes, a.dim, seed=1, clusters=12)
    rs.write_script(work, a.terminals)
    m = capi.Mmf([os.path.join(work, "hmmdefs")], hmm_list=os.path.join(work, "hmmlist"))
    occ, _ = capi.read_stats(m, os.path.join(work, "stats"))
    m.regtree(occ, 2)                                                        # (starts the HIP runtime, loads the kernels)
    t0 = time.perf_counter()
    t = m.regtree(occ, a.terminals)
    call = time.perf_counter() - t0
    iters, ms = t.stats()
    out = os.path.join(work, "lib"); os.makedirs(out)
    t.write(rs.IDENT, out)
    res = {"states": m.desc.numStates, "gaussians": m.desc.numGauss, "dim": a.dim, "terminals": t.num_terminals, "nodes": t.num_nodes,
           "call_s": round(call, 4), "kernel_s": round(ms / 1e3, 4), "kernel_share": round(ms / 1e3 / call, 3), "iterations": iters}
    if not a.no_hhed and os.path.exists(HHED):
        t0 = time.perf_counter(); run_hhed(work, "rc.hed", "."); full = time.perf_counter() - t0
        rs.write_script(work, 1, ident="none", name="ls.hed")
        t0 = time.perf_counter(); run_hhed(work, "ls.hed", out); load = time.perf_counter() - t0
        res["hhed_rc_s"] = round(full - load, 3); res["hhed_load_s"] = round(load, 3)
        res["identical"] = all(open(os.path.join(work, f), "rb").read() == open(os.path.join(out, f), "rb").read() for f in ("rtree.tree", "rtree.base"))
        res["speedup"] = round((full - load) / call, 2)
    shutil.rmtree(work)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
