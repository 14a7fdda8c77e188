"""Writes tests/golden/datacluster: HHEd edit scripts with TC / NC / TI commands and what the reference's HHEd (oracle/_ref/HHEd) makes of
them over the tree-clustering fixture's model set and statistics (tests/golden/treeclust: hmmdefs.gz, stats -- no new input set).

    python tests/golden/make_datacluster_golden.py        # needs oracle/_ref/HHEd; rewrites tests/golden/datacluster/

    a.hed  TC per centre phone and state                                   -> tied_a.mmf.gz
    b.hed  the same behind RO: the outlier phase merges groups, at least one into a group of LOWER slot number (trace.json)
                                                                           -> tied_b.mmf.gz
    c.hed  NC 4 per centre phone and state                                 -> tied_c.mmf.gz
    d.hed  TI on a .transP list and on a .state[2] list, over sub_untied.mmf.gz: the models of two centre phones with their
           transition matrices untied by the reference (UT)                -> tied_d.mmf.gz
    e.hed  TC over sub_mu2.mmf.gz: the same two centre phones after one MU 2 pass of the reference (the GDistance branch)
                                                                           -> tied_e.mmf.gz
The input set names one definition twice (a-a+c and b-a+c are twins): the commands over the a models hold a zero distance and a tie.
Thresholds are checked here: no command of (a) ends with everything apart or everything in one cluster, and the restatement of
tests/datacluster_util.py -- which must agree with HHEd's cluster trace -- says which commands of (b) merged into a lower slot."""
import gzip
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(HERE, "datacluster")
HHED = os.path.join(ROOT, "oracle", "_ref", "HHEd")

PHONES = list("abcdefghi")
SUB = "bc"
TC_THRESH, RO_THRESH, E_THRESH = 0.9, 60.0, 9.0


def script(which: str, ro=RO_THRESH) -> str:
    lines = []
    if which == "b":
        lines.append("RO %.1f stats" % ro)
    if which in "abc":
        for p in PHONES:
            for j in (2, 3, 4):
                if which == "c":
                    lines.append("NC 4 \"NC_%s_%d_\" {(\"*-%s+*\").state[%d]}" % (p, j, p, j))
                else:
                    lines.append("TC %.2f \"TC_%s_%d_\" {(\"*-%s+*\").state[%d]}" % (TC_THRESH, p, j, p, j))
    elif which == "d":
        lines.append("TI \"T_bc\" {(\"*-b+*\",\"*-c+*\").transP}")
        lines.append("TI \"S_b_2\" {\"*-b+*\".state[2]}")
    elif which == "e":
        for p in SUB:
            for j in (2, 3, 4):
                lines.append("TC %.2f \"GC_%s_%d_\" {(\"*-%s+*\").state[%d]}" % (E_THRESH, p, j, p, j))
    return "\n".join(lines) + "\n"


def run_hhed(workdir, mmf, lst, script_path, out_mmf, trace=0):
    r = subprocess.run([HHED, "-T", str(trace), "-H", mmf, "-w", out_mmf, script_path, lst], cwd=workdir, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        raise RuntimeError("HHEd failed:\n" + r.stdout[-3000:])
    return r.stdout


def sub_set(text: str) -> tuple:
    """The part of the model file that the two centre phones need (options, varFloor, their ~t macros, their models) and their list."""
    parts = re.split(r"^(?=~[a-z] )", text, flags=re.M)
    keep, names = [], []
    for blk in parts:
        m = re.match(r'~([a-z]) "([^"]+)"', blk)
        if blk.startswith("~o") or (m and m.group(1) == "v"):
            keep.append(blk)
        elif m and m.group(1) == "t" and m.group(2)[-1] in SUB:
            keep.append(blk)
        elif m and m.group(1) == "h" and m.group(2)[2] in SUB:
            keep.append(blk); names.append(m.group(2))
    return "".join(keep), names


def trace_clusters(out: str):
    """[(macro root, [[model, ...] per cluster])] from HHEd's -T 0400 cluster trace."""
    res = []
    for ln in out.splitlines():
        m = re.match(r"[TN]C \S+ (\S+) \{\}", ln.strip())
        if m:
            res.append((m.group(1), []))
        elif ln.startswith("  C.") and res:
            res[-1][1].append(ln.split("==" if "==" in ln else "]", 1)[1].split())
    return res


def main():
    import datacluster_util as du
    import treeclust_util as tu
    from htk_amd import capi
    if not os.path.exists(HHED):
        raise SystemExit("oracle/_ref/HHEd is missing: run build() where the reference lies")
    os.makedirs(OUT, exist_ok=True)
    work = tempfile.mkdtemp()
    mmf_path, lst = tu.unpack_inputs(work)
    shutil.copy(os.path.join(tu.G, "stats"), os.path.join(work, "stats"))
    base = capi.Mmf([mmf_path], hmm_list=lst)
    pk = base.packed()
    occ, _ = capi.read_stats(base, os.path.join(work, "stats"))
    trace = {}
    for which in "abc":
        open(os.path.join(OUT, which + ".hed"), "w").write(script(which))
        shutil.copy(os.path.join(OUT, which + ".hed"), work)
        out = run_hhed(work, "hmmdefs", "hmmlist", which + ".hed", "tied_%s.mmf" % which, trace=0o400)
        got = trace_clusters(out)
        assert len(got) == 27, len(got)
        # the restatement over the same items must name HHEd's clusters; it also knows what the trace does not say
        lower, counts = {}, {}
        for p in PHONES:
            for j in (2, 3, 4):
                il = base.item_list('{("*-%s+*").state[%d]}' % (p, j))
                st = [pk["hmmState"][pk["hmmStateOff"][h] + jj - 2] for h, jj in il]
                g = [pk["compGauss"][pk["stateCompOff"][s]] for s in st]
                d = du.divergence_matrix(pk["mean"][g], pk["var"][g])
                _, cv, low = du.ref_clustering(d, 4 if which == "c" else 1, 1.0e15 if which == "c" else TC_THRESH,
                                               occ[st] if which == "b" else None, RO_THRESH)
                root, clusters = got.pop(0)
                mine = [[base.phys_names[il[m][0]] for m in ch] for ch in cv]
                assert mine == clusters, (which, root, mine, clusters)
                counts[root] = len(cv)
                if which == "a":
                    assert 1 < len(cv) < len(il), (root, len(cv), len(il))
                if low:
                    lower[root] = low
        trace[which] = {"clusters": counts}
        if which == "b":
            assert lower, "no outlier merge into a lower slot: choose another RO threshold"
            trace[which]["lower_slot_outlier_merges"] = lower
    # (d), (e): the two centre phones' own set, through one pass of the reference each
    text, names = sub_set(open(mmf_path).read())
    open(os.path.join(work, "sub.mmf"), "w").write(text)
    open(os.path.join(work, "sublist"), "w").write("\n".join(names) + "\n")
    open(os.path.join(work, "ut.hed"), "w").write("UT {*.transP}\n")
    open(os.path.join(work, "mu.hed"), "w").write("MU 2 {*.state[2-4].mix}\n")
    run_hhed(work, "sub.mmf", "sublist", "ut.hed", "sub_untied.mmf")
    run_hhed(work, "sub.mmf", "sublist", "mu.hed", "sub_mu2.mmf")
    for which, inp in (("d", "sub_untied.mmf"), ("e", "sub_mu2.mmf")):
        open(os.path.join(OUT, which + ".hed"), "w").write(script(which))
        shutil.copy(os.path.join(OUT, which + ".hed"), work)
        out = run_hhed(work, inp, "sublist", which + ".hed", "tied_%s.mmf" % which, trace=0o400)
        if which == "e":
            got = trace_clusters(out)
            trace["e"] = {"clusters": {root: len(cl) for root, cl in got}}
            assert all(1 < len(cl) < 10 for _, cl in got), trace["e"]
    for name in ["tied_%s.mmf" % w for w in "abcde"] + ["sub_untied.mmf", "sub_mu2.mmf"]:
        with open(os.path.join(work, name), "rb") as f, gzip.GzipFile(os.path.join(OUT, name + ".gz"), "wb", mtime=0) as z:
            z.write(f.read())
    json.dump(trace, open(os.path.join(OUT, "trace.json"), "w"), indent=1, sort_keys=True)
    shutil.rmtree(work)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
