"""Writes tests/golden/regtree: small model sets with statistics files and `LS stats` + `RC N rtree [itemlist]` edit scripts
(tests/regtree_util.py: CASES), and what the reference's HHEd (oracle/_ref/HHEd) writes for them: rtree.tree and rtree.base.

    python tests/golden/make_regtree_golden.py        # needs oracle/_ref/HHEd; rewrites tests/golden/regtree/

Only the inputs (hmmdefs, hmmlist, stats, rc.hed) and HHEd's two output files are kept, one directory per case; a case of
regtree_util.NO_SPLIT adds a script <identifier>.hed and HHEd's <identifier>.tree / .base to its case's directory.  Checked here, on the
CPU: HHEd ends without an error on every case; a case's tree has the shape it is meant to have (b: 8 terminals from 70 / 130 Gaussians;
c: node 2 holds sil's Gaussians; d: fewer terminals than asked for; e: the two Gaussians at 0 share a class, and so does the pair with
identical means; f: the Gaussians without occupation are in some class; g: the tied state and the shared Gaussian appear once); h: HHEd's
cluster trace shows more than 10 iterations for the split.  iterations.json keeps the trace's iteration counts.

Beside each case's files, steps.npz keeps what the library's host side hands the device for the case, recomputed here from the parsed set
and the statistics file: the member arrays in the order of HHEd's own scan and the device steps (off, n, seeds) of the RC command (see
record_steps).  tests/test_regtree_ref.py reads them: they pin the float32 restatement of the kernels (tests/regtree_ref.py) to HHEd."""
import json
import os
import re
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

T_BID_CLUSTERS = 0o401       # T_BID's first bit + T_CLUSTERS (HHEd.c:75, :87): "Splitting Node" and "Iteration n: Distance" lines


def member_arrays(d, members):
    """What the host hands the device for the set in `d` (host/regtree.c, InitTreeAccs HHEd.c:2535): the rows of the Gaussians `members`
    = [(model, state, mixture), ...] in the order of InitRegTree's scan -- mean, the AccSum rows sum = mean x and sqr = (var + mean^2) x
    with x = the occupation of the first visited state with a positive one that holds the Gaussian, times its weight there; each product
    rounded to float."""
    import numpy as np
    from htk_amd import capi
    mmf = capi.Mmf([os.path.join(d, "hmmdefs")], hmm_list=os.path.join(d, "hmmlist"))
    pk = mmf.packed()
    socc, _ = capi.read_stats(mmf, os.path.join(d, "stats"))
    G, D = pk["numGauss"], pk["vecSize"]
    f32 = np.float32
    acc_occ, acc_sum, acc_sqr, hook = np.zeros(G, f32), np.zeros((G, D), f32), np.zeros((G, D), f32), np.zeros(G, bool)
    seen = set()
    for h in capi.hmm_scan_order(mmf.phys_names):
        for si in pk["hmmState"][pk["hmmStateOff"][h]:pk["hmmStateOff"][h + 1]]:
            if si in seen:
                continue
            seen.add(si)
            for c in range(pk["stateCompOff"][si], pk["stateCompOff"][si + 1]):
                g = pk["compGauss"][c]
                if not hook[g] and socc[si] > 0.0:
                    hook[g] = True
                    x = f32(socc[si]) * f32(pk["compWeight"][c])
                    acc_occ[g] = x
                    acc_sum[g] = pk["mean"][g] * x
                    acc_sqr[g] = (pk["var"][g] + pk["mean"][g] * pk["mean"][g]) * x
    gs = []
    for model, state, mix in members:
        h = mmf.phys_names.index(model)
        si = pk["hmmState"][pk["hmmStateOff"][h] + state - 2]
        gs.append(pk["compGauss"][pk["stateCompOff"][si] + mix - 1])
    assert len(set(gs)) == len(gs), "a Gaussian is listed twice"
    gs = np.array(gs)
    return pk["mean"][gs].astype(f32), acc_sum[gs], acc_sqr[gs], acc_occ[gs], hook[gs].astype(np.uint8)


def record_steps(ru, d, name, n, items, per_split):
    """<case>/steps.npz: the member arrays and the device steps (off, n, seeds) of the case's RC command.  The members' order is HHEd's own
    (the base classes of an RC that splits nothing, written to a scratch directory); the steps are tests/regtree_ref.py's, accepted only if
    they end in HHEd's tree, HHEd's classes and the iteration counts of HHEd's trace."""
    import tempfile
    import numpy as np
    import regtree_ref as rr
    with tempfile.TemporaryDirectory() as tmp:
        for f in ("hmmdefs", "hmmlist", "stats"):
            shutil.copy(os.path.join(d, f), tmp)
        ru.write_script(tmp, 2 if items else 1, items, ident="scan", name="scan.hed")
        ru.run_hhed(tmp, script="scan.hed")
        scan = ru.parse_base(open(os.path.join(tmp, "scan.base")).read())
    members = [m for cl in scan for m in cl]
    n_nonspeech = len(scan[0]) if items else 0
    mean, sum_, sqr, occ, has = member_arrays(d, members)
    ref = rr.RegTreeRef(mean, sum_, sqr, occ, has)
    steps, results, kids, ranges = rr.build_tree(ref, n, n_nonspeech)
    assert kids == ru.parse_tree(open(os.path.join(d, "rtree.tree")).read()), name
    classes = [[members[i] for i in ref.list[off:off + cnt]] for (l, r), (off, cnt) in zip(kids, ranges) if not l]
    assert classes == ru.parse_base(open(os.path.join(d, "rtree.base")).read()), name
    assert [int(r[0][2]) for s, r in zip(steps, results) if s[0] == "split"] == per_split, name
    D = mean.shape[1]
    np.savez_compressed(os.path.join(d, "steps.npz"), mean=mean, sum=sum_, sqr=sqr, occ=occ, has=has,
                        model=np.array([m[0] for m in members]), state=np.array([m[1] for m in members], np.int32),
                        mix=np.array([m[2] for m in members], np.int32), n_terminals=np.int32(n), n_nonspeech=np.int32(n_nonspeech),
                        step_split=np.array([s[0] == "split" for s in steps], np.uint8), step_off=np.array([s[1] for s in steps], np.int32),
                        step_n=np.array([s[2] for s in steps], np.int32),
                        step_seeds=np.array([s[3] if s[0] == "split" else np.zeros((2, D), np.float32) for s in steps], np.float32).reshape(len(steps), 2, D))


def main():
    import regtree_util as ru
    if not os.path.exists(ru.HHED):
        raise SystemExit("oracle/_ref/HHEd is missing: run build() where the reference lies")
    if os.path.isdir(ru.GOLDEN):
        shutil.rmtree(ru.GOLDEN)
    iters = {}
    for name in ru.CASES:
        d = os.path.join(ru.GOLDEN, name)
        n, items = ru.make_case(d, name)
        out = ru.run_hhed(d, trace=T_BID_CLUSTERS)
        assert "ERROR" not in out, out[-2000:]
        per_split, cur = [], 0
        for ln in out.splitlines():
            if ln.startswith("Splitting Node"):
                per_split.append(0)
            m = re.match(r"Iteration (\d+):", ln)
            if m and per_split:
                per_split[-1] = int(m.group(1))
        iters[name] = per_split
        kids = ru.parse_tree(open(os.path.join(d, "rtree.tree")).read())
        classes = ru.parse_base(open(os.path.join(d, "rtree.base")).read())
        nterm = sum(1 for k in kids if k == (0, 0))
        assert nterm == len(classes)
        total = sum(len(c) for c in classes)
        args = ru.CASES[name][0]
        full = len(args["names"]) * args["n_emit"] * args["n_mix"]
        print("%-5s N=%-3d nodes=%-3d terminals=%-3d gaussians=%-4d iterations=%s" % (name, n, len(kids), nterm, total, per_split))
        if name in ("b70", "b130"):
            assert total == (70 if name == "b70" else 130) and nterm == 8, (total, nterm)
        elif name == "a":
            assert total == 18 and nterm >= 2
        elif name == "c":
            assert kids[0] == (2, 3) and kids[1] == (0, 0) and all(c[0] == "sil" for c in classes[0]) and len(classes[0]) == 6, classes[0]
            assert nterm >= 3
        elif name == "d":
            assert 2 <= nterm < n
        elif name == "e":
            where = {c: k for k, cl in enumerate(classes) for c in cl}
            assert where[("m02", 3, 1)] == where[("m04", 4, 1)] and where[("m00", 2, 1)] == where[("m00", 2, 2)] and nterm >= 2
        elif name == "f":
            assert total == full and nterm >= 2
        elif name == "g":
            assert total == full - 2 - 1 and nterm >= 2, (total, full)
        elif name == "h":
            assert per_split and max(per_split) > 10, per_split
        record_steps(ru, d, name, n, items, per_split)
        kept = ["hmmdefs", "hmmlist", "stats", "rc.hed", "rtree.tree", "rtree.base", "steps.npz"]
        for (case, ident), (n2, items2) in ru.NO_SPLIT.items():
            if case != name:
                continue
            out = ru.run_hhed(d, trace=T_BID_CLUSTERS, script=ident + ".hed")
            assert "ERROR" not in out and "Splitting Node" not in out, out[-2000:]
            kids2 = ru.parse_tree(open(os.path.join(d, ident + ".tree")).read())
            classes2 = ru.parse_base(open(os.path.join(d, ident + ".base")).read())
            assert kids2 == ([(0, 0)] if n2 == 1 else [(2, 3), (0, 0), (0, 0)]) and sum(len(c) for c in classes2) == total, (kids2, total)
            print("%-5s %-8s classes of %s" % (name, ident, [len(c) for c in classes2]))
            if ident == "items":
                assert len(classes2[0]) == 2 * 14, classes2[0]
            kept += [ident + e for e in (".hed", ".tree", ".base")]
        for f in os.listdir(d):
            assert f in kept, f
    json.dump(iters, open(os.path.join(ru.GOLDEN, "iterations.json"), "w"), indent=1, sort_keys=True)
    print("wrote", ru.GOLDEN)


if __name__ == "__main__":
    main()
