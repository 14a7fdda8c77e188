"""HResults on the device: recognition output scored against reference transcriptions, every (reference, hypothesis) pair aligned side
by side in one call.

    python examples/hresults_score.py [-e class label] [-c] [-s] [-z name] [-n] [-f] [-t] [-p] [-I mlf] [-L dir] [-X ext] labelList recFiles...

The switches are HResults's own and the text is the reference's, line for line.  recFiles are label files, scored together as HResults
does, or master label files: a single one is scored entry by entry like HResults; SEVERAL (a decode grid: the same utterances recognised
under different settings) give one result block each, in the order given, from ONE device call.  --out FILE writes the text to FILE
instead of the standard output.  Word spotting (-w, -u), per-speaker results (-k), the NIST format (-h), N-best scoring (-d), file
limits (-m, -j) and the renaming of SENT / WORD (-a, -b) are refused by name."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htk_amd import capi

WITH_ARG = {"-z": 1, "-I": 1, "-L": 1, "-X": 1, "-e": 2, "--out": 1}


def parse(argv):
    o = dict(equiv=[], mlfs=[], flags=set(), z=None, L=None, X=None, out=None)
    k = 0
    while k < len(argv) and argv[k].startswith("-") and len(argv[k]) > 1:
        sw = argv[k]
        if sw != "--out":
            capi.results_check_switch(sw)                      # refuses what this path does not have, by name
        n = WITH_ARG.get(sw, 0)
        args = argv[k + 1:k + 1 + n]
        if len(args) < n:
            raise SystemExit("hresults_score: %s needs %d argument%s" % (sw, n, "" if n == 1 else "s"))
        if sw == "-e":
            o["equiv"].append((args[0], args[1]))
        elif sw == "-I":
            o["mlfs"].append(args[0])
        elif sw == "--out":
            o["out"] = args[0]
        elif n:
            o[sw[1]] = args[0]
        else:
            o["flags"].add(sw[1])
        k += 1 + n
    rest = argv[k:]
    if len(rest) < 1:
        raise SystemExit("hresults_score: the label list is missing")
    o["list"], o["rec"] = rest[0], rest[1:]
    return o


def is_mlf(path):
    with open(path, "rb") as f:
        return f.read(7) == b"#!MLF!#"


def entry_name(pattern):
    """The file name HResults scores an MLF entry under: a "*/name" pattern is kept as its name (HLabel.c, MLF_SIMPLE)."""
    rest = pattern[2:]
    return rest if pattern.startswith("*/") and not any(c in rest for c in "*?") else pattern


def read_list(path):
    return [ln.split()[0] for ln in open(path) if ln.split()]


def main(argv=None):
    o = parse(list(sys.argv[1:] if argv is None else argv))
    L = capi.lib()
    res = capi.Results(null_name=o["z"], equiv=o["equiv"], ignore_case="c" in o["flags"], strip="s" in o["flags"], nist="n" in o["flags"],
                       label_list=read_list(o["list"]))
    ref_mlfs = [capi.Mlf(p) for p in o["mlfs"]]
    ref_id = o["mlfs"][-1] if o["mlfs"] else o["L"]
    # the hypothesis sets: [(the arguments named on "Rec :", [(file name, id array)])]
    mlf_args = [p for p in o["rec"] if is_mlf(p)]
    sets = []
    if len(mlf_args) > 1 and len(mlf_args) == len(o["rec"]):
        for p in mlf_args:
            m = capi.Mlf(p)
            sets.append(([p], [(entry_name(pat), res.ids(h)) for pat, h in m.entries()]))
        names = [f for f, _ in sets[0][1]]
        for ids, files in sets[1:]:
            if [f for f, _ in files] != names:
                raise SystemExit("hresults_score: %s does not hold the utterances of %s in the same order" % (ids[0], sets[0][0][0]))
    else:
        files = []
        for p in o["rec"]:
            if is_mlf(p):
                m = capi.Mlf(p)
                files += [(entry_name(pat), res.ids(h)) for pat, h in m.entries()]
            else:
                h = capi.C.c_void_p()
                capi.check(L.htkamd_labels_read(p.encode(), capi.C.byref(h)), "labels_read")
                files.append((p, res.ids(h)))
                L.htkamd_labels_free(h)
        sets.append((o["rec"], files))
    rec_files = [f for f, _ in sets[0][1]]
    refs = [res.ref_for(f, ref_mlfs, o["L"], o["X"]) for f in rec_files]
    want_t, want_p = "t" in o["flags"], "p" in o["flags"]
    r = res.score([i for i, _ in refs], [[ids for _, ids in files] for _, files in sets], align=want_t, conf=want_p) if rec_files else None
    flags = (capi.RES_FULL if "f" in o["flags"] else 0) | (capi.RES_TRANS if want_t else 0) | (capi.RES_PSTATS if want_p else 0)
    U = len(rec_files)
    for k, (rec_ids, files) in enumerate(sets):
        for u in range(U):
            if r is not None and not r["counts"][k, u, 5]:
                print("hresults_score: %s or its reference %s is empty: left out" % (rec_files[u], refs[u][1]), file=sys.stderr)
        if r is None:
            res.write(flags, ref_id, rec_ids, [], [], [], [0] * 7, path=o["out"], append=k > 0)
            continue
        off = r["alnOff"][k * U:(k + 1) * U + 1] if want_t else None
        res.write(flags, ref_id, rec_ids, rec_files, [lf for _, lf in refs], r["counts"][k], r["totals"][k],
                  aln_off=None if off is None else off - off[0], aln=r["alnFlat"][off[0]:] if want_t else None,
                  conf=r["conf"][k] if want_p else None, path=o["out"], append=k > 0)
    sys.stdout.flush()
    return r


if __name__ == "__main__":
    main()
