"""Wall time of MLLR mean transforms over a synthetic set: the library's estimate from a pass's statistics (Mllr.estimate: class statistics,
tree sums and solves on the device) under three block layouts and, where oracle/_ref/HERest is built, the reference's HERest -u a on one
host core over the same files.

    python tools/mllr_bench.py [--states 5000] [--mixes 16] [--dim 39] [--terminals 32] [--files 1000] [--no-herest]

The set is regtree_bench's, the tree the library's own RC tree over it (the files HHEd would write), the speaker's files are drawn from the
set's Gaussians.  One library pass fills the statistics (pass_s); per layout call_s is the estimate alone (accumulators down, tables up,
three kernels, matrices back), kernel_s the device time of its kernels.  HERest's figure per layout is its run with -u a less its run with a
threshold above the root's occupation (the same pass and the same accumulation, no transform): what is left is ParseTree, AccNodeStats and
EstMLLRMeanXForm.  Prints one JSON line; max_dev is the largest difference between the two results' entries."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from htk_amd import capi, regtree_sets as rs, synth      # noqa: E402

HEREST = os.path.join(ROOT, "oracle", "_ref", "HERest")
THRESH = 500.0


def run_herest(work, blocks, thresh, out):
    open(os.path.join(work, "cfg"), "w").write(
        'HADAPT:TRANSKIND = MLLRMEAN\nHADAPT:ADAPTKIND = TREE\nHADAPT:REGTREE = rtree.tree\nHADAPT:BLOCKSIZE = "IntVec %d %s"\nHADAPT:USEBIAS = TRUE\n'
        "HADAPT:SPLITTHRESH = %f\nHMODEL:SAVEBINARY = FALSE\n" % (len(blocks), " ".join(map(str, blocks)), thresh))
    os.makedirs(os.path.join(work, out), exist_ok=True)
    t0 = time.perf_counter()
    subprocess.run([HEREST, "-C", "cfg", "-S", "train.scp", "-I", "labels.mlf", "-H", "hmmdefs", "-u", "a", "-J", ".", "-K", out, "mllr", "-h", "*/%%%_*", "hmmlist"],
                   cwd=work, check=True, stdout=subprocess.DEVNULL)
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--states", type=int, default=5000); ap.add_argument("--mixes", type=int, default=16); ap.add_argument("--dim", type=int, default=39)
    ap.add_argument("--terminals", type=int, default=32); ap.add_argument("--files", type=int, default=1000); ap.add_argument("--no-herest", action="store_true")
    a = ap.parse_args(argv)
    work = tempfile.mkdtemp()
    emit, D = 5, a.dim
    names = rs.names_for(max(a.states // emit, 1))
    rs.write_set(work, names, emit, a.mixes, D, seed=1, clusters=12)
    mmf = capi.Mmf([os.path.join(work, "hmmdefs")], hmm_list=os.path.join(work, "hmmlist"))
    occ, _ = capi.read_stats(mmf, os.path.join(work, "stats"))
    tree = mmf.regtree(occ, a.terminals)
    tree.write(rs.IDENT, work)
    pk = mmf.packed()
    model = capi.Model(pk)
    # the speaker's files: five models each, three frames per emitting state, from one of the state's Gaussians, shifted and scaled
    rng = np.random.RandomState(3)
    os.makedirs(os.path.join(work, "data"))
    feats, seqs, scp, mlf = [], [], [], ["#!MLF!#"]
    mean, var = np.asarray(pk["mean"]), np.asarray(pk["var"])
    for f in range(a.files):
        hs = rng.randint(0, len(names), size=5)
        gs = []
        for h in hs:
            for si in pk["hmmState"][pk["hmmStateOff"][h]:pk["hmmStateOff"][h + 1]]:
                c0, c1 = pk["stateCompOff"][si], pk["stateCompOff"][si + 1]
                gs += [pk["compGauss"][c] for c in rng.randint(c0, c1, size=3)]
        gs = np.array(gs)
        X = (0.95 * mean[gs] + 0.3 + rng.randn(len(gs), D) * np.sqrt(var[gs])).astype(np.float32)
        path = "data/sp1_f%04d.usr" % f
        synth.write_htk_param(os.path.join(work, path), X, kind=9)
        feats.append(X); seqs.append(np.array([mmf.logical[names[h]] for h in hs], np.int32)); scp.append(path)
        mlf += ['"*/sp1_f%04d.lab"' % f] + [names[h] for h in hs] + ["."]
    open(os.path.join(work, "train.scp"), "w").write("\n".join(scp) + "\n")
    open(os.path.join(work, "labels.mlf"), "w").write("\n".join(mlf) + "\n")
    batch = capi._Batch(feats, np.float32)
    fb, acc = capi.ForwardBackward(model), capi.Accs(model)
    fb.prepare(batch.dev.ptr.value, batch.off, capi.offsets([len(q) for q in seqs]), np.concatenate(seqs))
    t0 = time.perf_counter()
    fb.execute(capi.fb_config(), acc)
    ok = int((fb.results()[1] == 1).sum())
    pass_s = time.perf_counter() - t0
    layouts = [[D], [D // 3] * 3 if D % 3 == 0 else [D // 2, D - D // 2], [1, D - 1]]
    res = {"states": mmf.desc.numStates, "gaussians": mmf.desc.numGauss, "dim": D, "terminals": tree.num_terminals, "files": a.files,
           "frames": int(sum(len(x) for x in feats)), "utterances_ok": ok, "pass_s": round(pass_s, 3), "layouts": []}
    capi.Mllr.estimate(mmf, model, acc, tree, split_thresh=THRESH, blocks=[D])      # (loads the kernels)
    for blocks in layouts:
        t0 = time.perf_counter()
        xs = capi.Mllr.estimate(mmf, model, acc, tree, split_thresh=THRESH, blocks=blocks)
        call = time.perf_counter() - t0
        ms = xs.kernel_ms()
        row = {"blocks": blocks, "transforms": xs.num_xforms, "call_s": round(call, 4), "kernel_s": round(sum(ms) / 1e3, 4), "kernel_share": round(sum(ms) / 1e3 / call, 3),
               "stats_ms": round(ms[0], 2), "tree_ms": round(ms[1], 2), "solve_ms": round(ms[2], 2)}
        if not a.no_herest and os.path.exists(HEREST):
            full = run_herest(work, blocks, THRESH, "xf")
            base = run_herest(work, blocks, 1.0e9, "xf_none")
            ref = capi.Mllr.read(os.path.join(work, "xf", "sp1.mllr"))
            row.update(herest_s=round(full, 2), herest_pass_s=round(base, 2), herest_xform_s=round(full - base, 3), speedup=round((full - base) / call, 2),
                       same_classes=ref.class_xform == xs.class_xform)
            if row["same_classes"]:
                row["max_dev"] = float(max(max(np.abs(xs.xform(k)[0] - ref.xform(k)[0]).max(), np.abs(xs.xform(k)[1] - ref.xform(k)[1]).max())
                                           for k in range(1, xs.num_xforms + 1)))
        res["layouts"].append(row)
    shutil.rmtree(work)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
