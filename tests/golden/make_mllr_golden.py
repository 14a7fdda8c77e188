"""Writes tests/golden/mllr: one small adaptation task and what the reference's HERest -u a (oracle/_ref/HERest) makes of it.

    python tests/golden/make_mllr_golden.py        # needs oracle/_ref/HERest and oracle/_ref/HHEd; rewrites tests/golden/mllr/

The task: 8 three-state models with 2 mixture components, D = 6 (htk_amd/regtree_sets.py writes the set), HHEd's `RC 4` tree over it, and
one speaker: 30 short parameter files drawn here from the set's own Gaussians under a planted affine change of the means, with their
labels.  HERest runs one pass with HADAPT:TRANSKIND = MLLRMEAN, ADAPTKIND = TREE, BLOCKSIZE = "IntVec 2 2 4", USEBIAS = TRUE and writes
the speaker's transform file (-K).  Only data is kept: the set, lists, labels, parameter files, tree and base classes, the configuration
file, the reference's transform files and, in ref.json, its node occupations (HADAPT:TRACE's "Node n (occ)" lines) per threshold.

Thresholds (SPLITTHRESH), chosen from the node occupations of a first run so that the cases of tests/test_mllr_host.py exist:
  all      below every terminal: a transform per terminal
  one      between the smallest terminal and the next: that terminal's class goes to the nearest ancestor above the threshold
  subtree  above an inner node under the root: its classes go to the root
  none     above the root: no transform set
  equal    exactly the second smallest terminal's occupation (the trace's %f read back is the float): it counts as below, so it and its
           smaller sibling share their parent's transform; equalBelow, the next float down, gives it its own; equalRoot: no set
The main case is `one`; it is run a second time with the files in the opposite order, and 4 x the largest difference between the two
results (one figure, over every entry of every transform) is kept in ref.json as the tolerance of the device comparison, which floors it
at one float ulp of the entry: the reference sums its speaker statistics in float over the frames, so the order of the files is the
noise it carries itself.  That noise belongs to a row, not to an entry: where the two runs happen to print the same seven digits for an
entry, its neighbours in the row still differ.  Checked here:
in `one` a terminal does fall back, `equal` and `equalBelow` differ, and every class has 2 (largest block + 1) distinct means."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(HERE, "mllr")
HEREST = os.path.join(ROOT, "oracle", "_ref", "HERest")
D, BLOCKS, SPEAKER = 6, (2, 4), "sp1"
T_TRE = 0o10

CONFIG = """HADAPT:TRANSKIND = MLLRMEAN
HADAPT:ADAPTKIND = TREE
HADAPT:REGTREE = rtree.tree
HADAPT:BLOCKSIZE = "IntVec 2 2 4"
HADAPT:USEBIAS = TRUE
HADAPT:TRACE = %d
HMODEL:SAVEBINARY = FALSE
""" % T_TRE


def draw_files(d, names, rng):
    """The speaker's files: per file three models, four frames per emitting state, each frame from one of the state's two Gaussians
    (by its weight) with mean A mu + b."""
    from htk_amd import capi, synth
    mmf = capi.Mmf([os.path.join(d, "hmmdefs")], hmm_list=os.path.join(d, "hmmlist"))
    pk = mmf.packed()
    A = np.zeros((D, D))
    o = 0
    for bs in BLOCKS:
        A[o:o + bs, o:o + bs] = np.eye(bs) * 0.9 + 0.15 * rng.randn(bs, bs)
        o += bs
    b = 0.5 * rng.randn(D)
    os.makedirs(os.path.join(d, "data"), exist_ok=True)
    scp, mlf = [], ["#!MLF!#"]
    for f in range(30):
        seq = [names[k] for k in rng.randint(0, len(names), size=3)]
        rows = []
        for name in seq:
            h = mmf.phys_names.index(name)
            for si in pk["hmmState"][pk["hmmStateOff"][h]:pk["hmmStateOff"][h + 1]]:
                c0, c1 = pk["stateCompOff"][si], pk["stateCompOff"][si + 1]
                w = np.asarray(pk["compWeight"][c0:c1], np.float64)
                for _ in range(4):
                    g = pk["compGauss"][c0 + rng.choice(c1 - c0, p=w / w.sum())]
                    rows.append(A @ pk["mean"][g] + b + rng.randn(D) * np.sqrt(pk["var"][g]))
        path = "data/%s_f%02d.usr" % (SPEAKER, f)
        synth.write_htk_param(os.path.join(d, path), np.array(rows, np.float32), kind=9)
        scp.append(path)
        mlf += ['"*/%s_f%02d.lab"' % (SPEAKER, f)] + seq + ["."]
    open(os.path.join(d, "train.scp"), "w").write("\n".join(scp) + "\n")
    open(os.path.join(d, "train_rev.scp"), "w").write("\n".join(reversed(scp)) + "\n")
    open(os.path.join(d, "labels.mlf"), "w").write("\n".join(mlf) + "\n")


def run_herest(d, thresh, out_dir, scp="train.scp"):
    """One HERest -u a pass; returns ({node: occupation} from the trace, the transform file's text or None)."""
    cfg = os.path.join(d, "config.%s" % out_dir)
    open(cfg, "w").write(CONFIG + "HADAPT:SPLITTHRESH = %s\n" % thresh)
    os.makedirs(os.path.join(d, out_dir), exist_ok=True)
    r = subprocess.run([HEREST, "-C", os.path.basename(cfg), "-S", scp, "-I", "labels.mlf", "-H", "hmmdefs", "-u", "a", "-J", ".", "-K", out_dir, "mllr",
                        "-h", "*/%%%_*", "hmmlist"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    os.remove(cfg)
    if r.returncode:
        raise RuntimeError("HERest failed (%d):\n%s" % (r.returncode, r.stdout[-3000:]))
    occ = {int(m.group(1)): float(m.group(2)) for m in re.finditer(r"Node (\d+) \(([-0-9.e+]+)\)", r.stdout)}
    path = os.path.join(d, out_dir, SPEAKER + ".mllr")
    return occ, (open(path).read() if os.path.exists(path) else None), r.stdout


def parse_xforms(text):
    """(number of transforms, [transform of class 1..], [(bias[D], [block matrices])]) of a transform file's text."""
    tok = text.split()
    n = int(tok[tok.index("<NUMXFORMS>") + 1])
    cls = [int(m.group(2)) for m in re.finditer(r"<CLASSXFORM> (\d+) (\d+)", text)]
    xf = []
    for part in text.split("<LINXFORM>")[1:]:
        t = part.split("<XFORMWGTSET>")[0].split()
        i = t.index("<BIAS>")
        nb = int(t[i + 1])
        bias = [float(x) for x in t[i + 2:i + 2 + nb]]
        blocks = []
        for k, w in enumerate(t):
            if w == "<XFORM>":
                r, c = int(t[k + 1]), int(t[k + 2])
                blocks.append(np.array([float(x) for x in t[k + 3:k + 3 + r * c]]).reshape(r, c))
        xf.append((np.array(bias), blocks))
    assert len(xf) == n
    return n, cls, xf


def main():
    import regtree_util as ru
    from htk_amd import regtree_sets
    if not (os.path.exists(HEREST) and os.path.exists(ru.HHED)):
        raise SystemExit("oracle/_ref/HERest or HHEd is missing: run build() where the reference lies")
    if os.path.isdir(GOLDEN):
        shutil.rmtree(GOLDEN)
    d = GOLDEN
    names = regtree_sets.names_for(8)
    regtree_sets.write_set(d, names=names, n_emit=3, n_mix=2, D=D, seed=41)
    regtree_sets.write_script(d, 4)
    ru.run_hhed(d)
    kids = ru.parse_tree(open(os.path.join(d, "rtree.tree")).read())
    classes = ru.parse_base(open(os.path.join(d, "rtree.base")).read())
    assert len(kids) == 7 and len(classes) == 4, kids
    rng = np.random.RandomState(7)
    draw_files(d, names, rng)
    open(os.path.join(d, "config"), "w").write(CONFIG)

    occ, text, _ = run_herest(d, "1.0", "xf_probe")
    shutil.rmtree(os.path.join(d, "xf_probe"))
    term = sorted(n for n in occ if kids[n - 1] == (0, 0))
    tocc = sorted(occ[n] for n in term)
    inner = [n for n in occ if kids[n - 1] != (0, 0) and n != 1]
    thresholds = {"all": "%.3f" % (tocc[0] * 0.5), "one": "%.3f" % (0.5 * (tocc[0] + tocc[1])),
                  "subtree": "%.3f" % (min(occ[n] for n in inner) + 0.5), "none": "%.3f" % (occ[1] + 1.0)}
    # an occupation exactly on the threshold: the trace's %f is finer than a float's spacing here, so the printed figure read back is the
    # float itself.  `equal`: the second smallest terminal on the threshold (it and its smaller sibling fall to their parent: another class
    # map than just below it, `equalBelow`, the next float down, where it keeps its own transform); `equalRoot`: the root on it, no set
    eq = sorted(term, key=lambda n: occ[n])[1]
    assert float(np.float32(float("%f" % occ[eq]))) == float(np.float32(occ[eq]))
    thresholds["equal"] = "%f" % occ[eq]
    thresholds["equalBelow"] = "%.9f" % float(np.nextafter(np.float32(occ[eq]), np.float32(0.0)))
    thresholds["equalRoot"] = "%f" % occ[1]
    ref = {"blocks": list(BLOCKS), "speaker": SPEAKER, "children": kids, "cases": {}}
    for name, th in thresholds.items():
        o, text, out = run_herest(d, th, "xf_" + name)
        case = {"thresh": float(th), "nodeOcc": {str(k): v for k, v in sorted(o.items())}}
        if text is None:
            case.update(numXforms=0, classXform=[])
            shutil.rmtree(os.path.join(d, "xf_" + name))
        else:
            n, cls, _ = parse_xforms(text)
            case.update(numXforms=n, classXform=cls)
        ref["cases"][name] = case
        print("%-8s thresh %-10s transforms %d classes %s" % (name, th, case["numXforms"], case["classXform"]))
    one = ref["cases"]["one"]
    ref["equalNode"] = eq
    assert ref["cases"]["equal"]["classXform"] != ref["cases"]["equalBelow"]["classXform"], "the threshold did not land on the float"
    assert ref["cases"]["equalBelow"]["classXform"] == one["classXform"] and ref["cases"]["equalRoot"]["numXforms"] == 0
    # `one`: the smallest terminal is below the threshold, so the transform of its class is its parent's (estimated from both children's
    # statistics, used by that class alone): still one transform per class, another matrix for that class, the same for the others
    assert ref["cases"]["all"]["numXforms"] == 4 and one["numXforms"] == 4 and ref["cases"]["none"]["numXforms"] == 0, one
    small = min(term, key=lambda n: occ[n])
    xs_all = parse_xforms(open(os.path.join(d, "xf_all", SPEAKER + ".mllr")).read())
    xs_one = parse_xforms(open(os.path.join(d, "xf_one", SPEAKER + ".mllr")).read())
    for k, n in enumerate(term):
        same = np.array_equal(xs_all[2][xs_all[1][k] - 1][0], xs_one[2][xs_one[1][k] - 1][0])
        assert same == (n != small), (n, small)
    ref["fallback"] = {"terminal": small, "class": term.index(small) + 1}
    # no singular class: every class has at least 2 (largest block + 1) distinct means
    text = open(os.path.join(d, "hmmdefs")).read()
    means = {}
    for hm in re.finditer(r'~h "([^"]+)"(.*?)<ENDHMM>', text, re.S):
        for st in re.finditer(r"<STATE> (\d+)(.*?)(?=<STATE>|<TRANSP>)", hm.group(2), re.S):
            for mx in re.finditer(r"<MIXTURE> (\d+) \S+\s*<MEAN> \d+\s*([^<]+)", st.group(2)):
                means[(hm.group(1), int(st.group(1)), int(mx.group(1)))] = tuple(mx.group(2).split())
    for cl in classes:
        assert len({means[c] for c in cl}) >= 2 * (max(BLOCKS) + 1), len(cl)
    # the reference's own noise: the same pass with the files in the opposite order
    _, text_a, _ = run_herest(d, thresholds["one"], "xf_one")
    _, text_b, _ = run_herest(d, thresholds["one"], "xf_one_rev", scp="train_rev.scp")
    na, ca, xa = parse_xforms(text_a)
    nb, cb, xb = parse_xforms(text_b)
    assert (na, ca) == (nb, cb)
    largest = 0.0
    for (ba, ma), (bb, mb) in zip(xa, xb):
        largest = max([largest, float(np.abs(ba - bb).max())] + [float(np.abs(p - q).max()) for p, q in zip(ma, mb)])
    assert largest > 0.0
    ref["largestDifference"] = largest          # between the reference's two file orders, over every entry of every transform
    ref["bound"] = 4.0 * largest                # the test floors it at one float ulp of the entry
    print("largest difference between the two file orders %.3g: bound %.3g" % (largest, 4.0 * largest))
    shutil.rmtree(os.path.join(d, "xf_one_rev"))
    os.remove(os.path.join(d, "train_rev.scp"))
    json.dump(ref, open(os.path.join(d, "ref.json"), "w"), indent=1, sort_keys=True)
    print("wrote", d)


if __name__ == "__main__":
    main()
