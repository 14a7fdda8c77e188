"""Writes tests/golden/regtree: small model sets with statistics files and `LS stats` + `RC N rtree [itemlist]` edit scripts
(tests/regtree_util.py: CASES), and what the reference's HHEd (oracle/_ref/HHEd) writes for them: rtree.tree and rtree.base.

    python tests/golden/make_regtree_golden.py        # needs oracle/_ref/HHEd; rewrites tests/golden/regtree/

Only the inputs (hmmdefs, hmmlist, stats, rc.hed) and HHEd's two output files are kept, one directory per case; a case of
regtree_util.NO_SPLIT adds a script <identifier>.hed and HHEd's <identifier>.tree / .base to its case's directory.  Checked here, on the
CPU: HHEd ends without an error on every case; a case's tree has the shape it is meant to have (b: 8 terminals from 70 / 130 Gaussians;
c: node 2 holds sil's Gaussians; d: fewer terminals than asked for; e: the two Gaussians at 0 share a class, and so does the pair with
identical means; f: the Gaussians without occupation are in some class; g: the tied state and the shared Gaussian appear once); h: HHEd's
cluster trace shows more than 10 iterations for the split.  iterations.json keeps the trace's iteration counts."""
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
        kept = ["hmmdefs", "hmmlist", "stats", "rc.hed", "rtree.tree", "rtree.base"]
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
