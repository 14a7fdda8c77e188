"""Fixture of tests/test_treeclust_host.py and tests/test_gpu_treeclust.py: a synthetic single-Gaussian triphone set, its HERest -s
statistics file, three HHEd edit scripts (RO / QS / TB / ST) and what the reference's HHEd (oracle/_ref/HHEd) makes of them.

    python tests/golden/make_treeclust_golden.py          # needs oracle/_ref/HHEd; rewrites tests/golden/treeclust/

The set: 9 phones, 5-state models (3 emitting), D = 5.  Centre phone `a` has all 81 contexts (a tree root of more than 64 items), the
others 10 each.  Means depend on the class of the left and of the right context plus noise, so that trees get several levels.  There is
a varFloor1 macro, a few states have no occupation, and two models have identical statistics.  The functions are also used by the live
check of the GPU test (a second seed for the occupations).
"""
from __future__ import annotations

import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "treeclust")
HHED = os.path.join(ROOT, "oracle", "_ref", "HHEd")

PHONES = list("abcdefghi")
CLASSES = {"Vowel": "aei", "Stop": "bdg", "Fric": "cfh"}
D, NEMIT = 5, 3
RO_THRESH, TB_THRESH = 40.0, 12.0


def fmt(v):
    return "%e" % float(v)


def models():
    names = ["%s-a+%s" % (l, r) for l in PHONES for r in PHONES]
    rng = np.random.RandomState(5)
    for p in PHONES[1:]:
        ctx = [(l, r) for l in PHONES for r in PHONES]
        rng.shuffle(ctx)
        names += ["%s-%s+%s" % (l, p, r) for l, r in ctx[:10]]
    return names


def cls(ph):
    return [k for k, v in enumerate(CLASSES.values()) if ph in v][0]


def write_set(mmf_path, list_path):
    """The text MMF (~o, ~v varFloor1, one ~t per centre phone, the models) and the HMM list, in the same order."""
    rng = np.random.RandomState(7)
    names = models()
    base = {p: rng.randn(NEMIT, D) * 2.0 for p in PHONES}
    loff = rng.randn(3, NEMIT, D) * 1.2
    roff = rng.randn(3, NEMIT, D) * 1.2
    with open(mmf_path, "w") as f:
        f.write("~o\n<STREAMINFO> 1 %d\n<VECSIZE> %d<NULLD><USER><DIAGC>\n" % (D, D))
        f.write("~v \"varFloor1\"\n<VARIANCE> %d\n %s\n" % (D, " ".join(fmt(0.05 + 0.01 * k) for k in range(D))))
        for p in PHONES:
            f.write("~t \"T_%s\"\n<TRANSP> 5\n 0.0 1.0 0.0 0.0 0.0\n 0.0 0.6 0.4 0.0 0.0\n 0.0 0.0 0.6 0.4 0.0\n 0.0 0.0 0.0 0.7 0.3\n 0.0 0.0 0.0 0.0 0.0\n" % p)
        for n in names:
            l, p, r = n[0], n[2], n[4]
            f.write("~h \"%s\"\n<BEGINHMM>\n<NUMSTATES> 5\n" % n)
            if n == "b-a+c":                              # the twin of a-a+c (the model before it in the list has other contexts)
                mean, var = twin
            else:
                # the left context shapes the first states, the right context the last
                w = np.array([1.0, 0.5, 0.1])[:, None]
                mean = base[p] + w * loff[cls(l)] + w[::-1] * roff[cls(r)] + rng.randn(NEMIT, D) * 0.25
                var = 0.4 + rng.rand(NEMIT, D) * 0.8
            if n == "a-a+c":
                twin = (mean, var)
            for j in range(NEMIT):
                m32 = np.array([float(fmt(x)) for x in mean[j]], np.float32); v32 = np.array([float(fmt(x)) for x in var[j]], np.float32)
                gc = np.float32(D * np.log(2 * np.pi) + np.sum(np.log(v32.astype(np.float64))))
                f.write("<STATE> %d\n<MEAN> %d\n %s\n<VARIANCE> %d\n %s\n<GCONST> %s\n" % (j + 2, D, " ".join(fmt(x) for x in m32), D, " ".join(fmt(x) for x in v32), fmt(gc)))
            f.write("~t \"T_%s\"\n<ENDHMM>\n" % p)
    with open(list_path, "w") as f:
        f.write("\n".join(names) + "\n")
    return names


def write_stats(mmf, path, seed):
    """The statistics file through the library's own writer: random occupations, a few of them zero, the twins alike."""
    from htk_amd import capi
    rng = np.random.RandomState(seed)
    pk = mmf.packed()
    lay = capi.accs_layout(pk)
    vec = np.zeros(lay.total, np.float64)
    H = pk["numPhys"]
    occ = (3.0 + rng.rand(H, NEMIT) * 60.0).astype(np.float32)
    for k in rng.choice(H * NEMIT, 7, replace=False):
        occ.reshape(-1)[k] = 0.0
    ia, ib = mmf.phys_names.index("a-a+c"), mmf.phys_names.index("b-a+c")
    occ[ib] = occ[ia]
    for h in range(H):
        vec[lay.nEgs + h] = 1 + int(occ[h].sum() / 10)
        for j in range(NEMIT):
            vec[lay.wtOcc + pk["hmmState"][pk["hmmStateOff"][h] + j]] = occ[h, j]
    capi.stats_write_file(pk, vec, mmf.phys_names, path)


def questions():
    q = []
    for side, pat in (("L", "%s-*"), ("R", "*+%s")):
        for cname, members in CLASSES.items():
            q.append(("%s_%s" % (side, cname), [pat % m for m in members]))
        for ph in "abcd":
            q.append(("%s_%s" % (side, ph), [pat % ph]))
    q.insert(1, ("L_Vowel_again", ["i-*", "a-*", "e-*"]))            # another name for L_Vowel's answers: L_Vowel must win
    q.append(("C_a", ["*-a+*"]))                                      # true for every model of a's trees, for none of the others'
    q.append(("L_z", ["z-*"]))                                        # answers for no model at all: dropped with a warning
    q.append(("R_notVowel", ["*+b", "*+c", "*+d", "*+f", "*+g", "*+h"]))
    return q


def script(which: int, stats="stats", trees="trees") -> str:
    thr = 1.0e9 if which == 3 else TB_THRESH
    lines = ["RO %.1f %s" % (RO_THRESH, stats), "TR 0"]
    for name, pats in questions():
        lines.append("QS '%s' { %s }" % (name, ",".join('"%s"' % p for p in pats)))
    lines.append("TR 4")
    for p in PHONES:
        for j in range(2, 2 + NEMIT):
            lines.append("TB %.1f \"ST_%s_%d_\" {(\"*-%s+*\").state[%d]}" % (thr, p, j, p, j))
    lines += ["TR 0", "ST %s" % trees]
    return "\n".join(lines) + "\n"


def run_hhed(workdir, mmf_path, list_path, script_path, out_mmf, config=None, trace=0):
    cmd = [HHED, "-T", str(trace), "-H", mmf_path, "-w", out_mmf]
    if config:
        cmd[1:1] = ["-C", config]
    r = subprocess.run(cmd + [script_path, list_path], cwd=workdir, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        raise RuntimeError("HHEd failed:\n" + r.stdout[-3000:])
    return r.stdout


def split_trace(out: str):
    """[(tree, [question of split 0, 1, ...])] from HHEd's -T trace (" Start  p[j]" ... "  Split ..." + the question's line)."""
    trees, cur = [], None
    lines = out.splitlines()
    for k, ln in enumerate(lines):
        m = re.match(r"\s*Start\s+(\S+)\[(\d)\]", ln)
        if m:
            cur = ["%s[%s]" % (m.group(1), m.group(2)), []]
            trees.append(cur)
        elif re.match(r"\s*Split ", ln) and cur is not None:
            cur[1].append(lines[k + 1].split()[0])
    return trees


def main():
    from htk_amd import capi
    if not os.path.exists(HHED):
        raise SystemExit("oracle/_ref/HHEd is missing: run build() where the reference lies")
    os.makedirs(OUT, exist_ok=True)
    mmf_path, list_path = os.path.join(OUT, "hmmdefs"), os.path.join(OUT, "hmmlist")
    write_set(mmf_path, list_path)
    mmf = capi.Mmf([mmf_path], hmm_list=list_path)
    write_stats(mmf, os.path.join(OUT, "stats"), 11)
    with open(os.path.join(OUT, "config2"), "w") as f:
        f.write("TREEMERGE = F\nUSELEAFSTATS = F\n")
    info = {}
    for which in (1, 2, 3):                                           # script 2 is script 1 under config2
        sname = "script%d.hed" % (1 if which == 2 else which)
        with open(os.path.join(OUT, sname), "w") as f:
            f.write(script(which, trees="trees"))
        out = run_hhed(OUT, "hmmdefs", "hmmlist", sname, "tied%d.mmf" % which, config="config2" if which == 2 else None, trace=1)
        os.replace(os.path.join(OUT, "trees"), os.path.join(OUT, "trees%d" % which))
        if which == 1:
            tr = split_trace(out)
            merges = len(re.findall(r"BestM ", out))
            with open(os.path.join(OUT, "trace1.json"), "w") as f:
                f.write(json.dumps({"merges": merges, "splits": tr}).replace("], [", "],\n["))
            info = {"levels": 0, "merges": merges}
            # levels from the trees file: a node whose child is a node whose child is a node
            txt = open(os.path.join(OUT, "trees1")).read()
            for blk in re.findall(r"\{\n(.*?)\}", txt, flags=re.S):
                kids = {}
                for ln in blk.strip().splitlines():
                    f4 = ln.split()
                    kids[int(f4[0])] = [int(x) for x in f4[2:4] if re.fullmatch(r"-?\d+", x)]
                def depth(n):
                    return 1 + max([depth(c) for c in kids.get(n, [])] + [0])
                info["levels"] = max(info["levels"], depth(0))
            assert info["levels"] >= 3, "no tree of script 1 has three levels: the fixture tests nothing (%s)" % info
            assert merges >= 1, "script 1 merges no pair of leaves: the fixture tests nothing"
    # the order of an item list and a question's answers as HHEd sees them (-T 8: PState prints the models it walks, PHIdent the names it finds)
    with open(os.path.join(OUT, "probe.hed"), "w") as f:
        f.write("TR 8\nQS 'L_Stop' { \"b-*\",\"d-*\",\"g-*\" }\nTR 0\nRO 1.0 stats\nTR 8\nTB 1.0e9 \"X_\" {(\"*-a+*\",\"*-b+*\").state[3]}\n")
    out = run_hhed(OUT, "hmmdefs", "hmmlist", "probe.hed", os.path.join(OUT, "probe.out"), trace=0)
    os.remove(os.path.join(OUT, "probe.out")); os.remove(os.path.join(OUT, "probe.hed"))
    walked = re.findall(r"^\s+(\S+)\.state\[3\]\s*$", out, flags=re.M)
    lines = out.splitlines()
    blocks = [lines[k + 1].split() for k, ln in enumerate(lines) if ln.startswith(" Models")]
    qnames = sum(blocks[:3], [])                                      # the question's three item sets come first, then TB's one
    with open(os.path.join(OUT, "probe.json"), "w") as f:
        json.dump({"question": ["b-*", "d-*", "g-*"], "answers_true": sorted(qnames), "item_list": "{(\"*-a+*\",\"*-b+*\").state[3]}",
                   "pstate_walk": walked}, f)
    # the model sets are kept compressed (they are most of the fixture's bytes); the list is the models' names in definition order
    for n in ("hmmdefs", "tied1.mmf", "tied2.mmf", "tied3.mmf"):
        with open(os.path.join(OUT, n), "rb") as f, open(os.path.join(OUT, n + ".gz"), "wb") as g:
            with gzip.GzipFile(filename="", mode="wb", fileobj=g, mtime=0) as z:
                z.write(f.read())
        os.remove(os.path.join(OUT, n))
    os.remove(os.path.join(OUT, "hmmlist"))
    print("treeclust golden:", info, {n: os.path.getsize(os.path.join(OUT, n)) for n in sorted(os.listdir(OUT))})


if __name__ == "__main__":
    main()
