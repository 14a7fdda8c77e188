"""HLRescore on the device: a batch of lattices rescored, pruned and written under one setting or a whole grid of them.

    python examples/hlrescore_batch.py [-C cfg] [-f] [-w] [-t f [a]] [-u f [a]] [-s f] [-p f] [-a f] [-r f] [-i mlf] [-l dir] [-y ext] [-o fmt]
                                       [-L dir] [-X ext] [-q fmt] [-T 1] [--grid "s=..;p=.."] [-I ref.mlf] dictionary lattices...

The switches are HLRescore's own and the files are the reference's, byte for byte; -C reads STARTWORD, ENDWORD and SORTLATTICE.
--grid "s=5,10,15;p=0,-5" runs EVERY combination of the listed values of -s -p -a -r in one device call; the outputs of combination k go
to <dir>/k<k>/ (-l) or <mlf>.k<k> (-i), and with -I ref.mlf one HResults block per combination is printed, scored in one further call
with no file in between.  -n / -wn, -m, -c, -I as label input, -d, -P and FIXBADLATS are refused by name."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htk_amd import capi

WITH_ARG = {"-C": 1, "-s": 1, "-p": 1, "-a": 1, "-r": 1, "-i": 1, "-l": 1, "-y": 1, "-o": 1, "-L": 1, "-X": 1, "-q": 1, "-T": 1, "--grid": 1, "-I": 1}


def is_float(s):
    try:
        float(s)
        return True
    except ValueError:
        return False


def read_config(path, o):
    for line in open(path):
        line = line.split("#")[0].strip()
        if "=" not in line:
            continue
        name, val = [x.strip() for x in line.split("=", 1)]
        mod, _, name = name.rpartition(":")
        if mod.strip() not in ("", "HLRESCORE"):
            continue
        name = name.strip()
        if name in ("STARTWORD", "ENDWORD"):
            o[name] = val.strip('"')
        elif name == "SORTLATTICE":
            o["sort"] = val[:1] in "Tt"
        elif name == "FIXBADLATS" and val[:1] in "Tt":
            capi.latset_check_switch("FIXBADLATS")


def parse(argv):
    o = dict(flags=set(), s=1.0, p=0.0, a=1.0, r=1.0, i=None, l=None, y="rec", o=None, L=None, X="lat", q=None, T=0, grid=None, ref=None, t=None, u=None,
             STARTWORD=None, ENDWORD=None, sort=True)
    k = 0
    while k < len(argv) and argv[k].startswith("-") and len(argv[k]) > 1 and not is_float(argv[k]):
        sw = argv[k]
        if sw == "-I" and not any(a == "--grid" for a in argv):
            capi.latset_check_switch("-I")                       # label input: refused by name
        if sw not in ("--grid", "-I"):
            capi.latset_check_switch(sw)
        if sw in ("-t", "-u"):
            if k + 1 >= len(argv) or not is_float(argv[k + 1]):
                raise SystemExit("HLRescore:  lattice pruning threshold expected")
            v = [float(argv[k + 1]), 0.0]
            k += 2
            if k < len(argv) and is_float(argv[k]) and ("." in argv[k] or "e" in argv[k].lower()):
                v[1] = float(argv[k]); k += 1
            o[sw[1]] = v
            continue
        n = WITH_ARG.get(sw, 0)
        if len(argv) < k + 1 + n:
            raise SystemExit("hlrescore_batch: %s needs an argument" % sw)
        if sw == "-C":
            read_config(argv[k + 1], o)
        elif sw == "--grid":
            o["grid"] = argv[k + 1]
        elif sw == "-I":
            o["ref"] = argv[k + 1]
        elif sw in ("-s", "-p", "-a", "-r"):
            o[sw[1]] = float(argv[k + 1])
        elif sw == "-T":
            o["T"] = int(argv[k + 1])
        elif n:
            o[sw[1]] = argv[k + 1]
        else:
            o["flags"].add(sw[1])
        k += 1 + n
    if not ({"w", "f"} & o["flags"]):
        raise SystemExit("HLRescore: No operation specified. What do you want me to do?")
    if len(argv) - k < 1:
        raise SystemExit("Vocab file name expected")
    o["dict"], o["files"] = argv[k], argv[k + 1:]
    return o


def make_fn(fn, directory, ext):
    """MakeFN (HShell.c): the file's own directory unless one is given, its extension replaced."""
    d, base = os.path.split(fn)
    base = os.path.splitext(base)[0] + ("." + ext if ext else "")
    d = directory if directory is not None else d
    return os.path.join(d, base) if d else base


def settings_of(o):
    """[(a, s, p, r)] -- one, or every combination of the grid."""
    if not o["grid"]:
        return [(o["a"], o["s"], o["p"], o["r"])]
    axes = dict(a=[o["a"]], s=[o["s"]], p=[o["p"]], r=[o["r"]])
    for part in o["grid"].split(";"):
        if part.strip():
            name, vals = part.split("=")
            if name.strip() not in axes:
                raise SystemExit("hlrescore_batch: --grid knows s p a r, not %s" % name)
            axes[name.strip()] = [float(v) for v in vals.split(",")]
    return [(a, s, p, r) for s, p, a, r in itertools.product(axes["s"], axes["p"], axes["a"], axes["r"])]


def pruned_sets(base, sets, settings, beam):
    """LatPrune per setting: sets[k] (base itself where nothing was pruned yet) -> a new set per setting."""
    out = []
    if all(s is base for s in sets):
        pr = base.prune(settings, beam[0], beam[1])               # every setting in one call
        todo = [(base, pr["keep_node"][k], pr["keep_arc"][k]) for k in range(len(settings))]
    else:
        todo = []
        for k, s in enumerate(sets):
            pr = s.prune([settings[k]], beam[0], beam[1])
            todo.append((s, pr["keep_node"][0], pr["keep_arc"][0]))
    for src, kn, ka in todo:
        dst = capi.LatSet(like=src)
        for u in range(len(src)):
            dst.add_pruned(src, u, kn[u], ka[u])
        out.append(dst)
    return out


def main(argv=None):
    o = parse(list(sys.argv[1:] if argv is None else argv))
    settings = settings_of(o)
    K, grid = len(settings), o["grid"] is not None
    base = capi.LatSet(o["dict"], o["STARTWORD"], o["ENDWORD"])
    for f in o["files"]:
        if o["T"] & 1:
            print("File: %s" % f)
        base.add_file(make_fn(f, o["L"], o["X"]))
    U = len(base)
    sets = [base] * K
    if U == 0:
        return None
    if o["t"]:
        sets = pruned_sets(base, sets, settings, o["t"])
    best = None
    if "f" in o["flags"]:
        if all(s is base for s in sets):
            best = base.best(settings)                              # K x U in one call
            paths = best["paths"]
        else:
            paths = [s.best([settings[k]])["paths"][0] for k, s in enumerate(sets)]
        for k in range(K):
            mlf = capi.MlfOut(o["i"] + (".k%d" % k if grid else "")) if o["i"] else None
            ldir = o["l"] if not grid or o["l"] is None else os.path.join(o["l"], "k%d" % k)
            if grid and ldir and not os.path.isdir(ldir):
                os.makedirs(ldir)
            for u, f in enumerate(o["files"]):
                tr = sets[k].trans(u, settings[k], paths[k][u])
                if o["o"]:
                    tr.format(frame_dur=1.0e7, flags=o["o"])
                name = make_fn(f, ldir, o["y"])
                if mlf:
                    mlf.add(name, tr)
                else:
                    tr.write(name)
            if mlf:
                mlf.close()
    if o["u"]:
        sets = pruned_sets(base, sets, settings, o["u"])
    if "w" in o["flags"]:
        for k in range(K):
            ldir = o["l"] if not grid or o["l"] is None else os.path.join(o["l"], "k%d" % k)
            if grid and ldir and not os.path.isdir(ldir):
                os.makedirs(ldir)
            fb = sets[k].fb_max([settings[k]]) if o["sort"] else None      # LatSetScores
            for u, f in enumerate(o["files"]):
                score = None if fb is None else fb["fw"][u][:, 0] + fb["bw"][u][:, 0]
                sets[k].write(u, settings[k], make_fn(f, ldir, o["X"]), node_score=score, fmt=o["q"])
    report = None
    if o["ref"] and "f" in o["flags"]:
        res = capi.Results()
        ref = capi.Mlf(o["ref"])
        names = [make_fn(f, None, o["y"]) for f in o["files"]]
        refs = [res.ref_for(n, [ref]) for n in names]
        if best is not None:
            hyps = base.best_ids(res, best)                         # lattices -> K hypothesis sets with no file in between
        else:
            hyps = [s.best_ids(res, s.best([settings[k]]))[0] for k, s in enumerate(sets)]
        report = res.score([i for i, _ in refs], hyps)
        for k in range(K):
            print("==== setting %d: -a %g -s %g -p %g -r %g" % ((k,) + settings[k]))
            sys.stdout.flush()
            res.write(0, o["ref"], [o["i"] or o["l"] or "lattices"], names, [lf for _, lf in refs], report["counts"][k], report["totals"][k])
    sys.stdout.flush()
    return dict(settings=settings, best=best, report=report)


if __name__ == "__main__":
    main()
