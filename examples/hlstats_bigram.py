"""HLStats on the device: label files counted in one call, bigram models and listings written as the reference writes them.

    python examples/hlstats_bigram.py [-b fn] [-o] [-t n] [-u f] [-f f] [-s s1 s2] [-c N] [-d] [-l fn] [-I mlf] [-G fmt] [-L dir] [-X ext] wordList labFiles...

The switches are HLStats's own; labFiles are label files (found through -I mlf, -L dir and -X ext as HLStats finds them) or master
label files, whose every entry is counted.  --discount D stands for the DISCOUNT configuration value,
--trace FILE receives the lines HLStats -T 4 prints, --out FILE the standard output.  -p and -h are refused by name."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htk_amd import capi

WITH_ARG = {"-b": 1, "-t": 1, "-u": 1, "-f": 1, "-s": 2, "-c": 1, "-l": 1, "-I": 1, "-G": 1, "-L": 1, "-X": 1, "--discount": 1, "--trace": 1, "--out": 1}


def main(argv):
    o, k = {}, 0
    while k < len(argv) and argv[k].startswith("-") and len(argv[k]) > 1:
        sw = argv[k]
        if not sw.startswith("--"):
            capi.check(capi.lib().htkamd_lstats_check_switch(sw.encode()), "hlstats_bigram")
        n = WITH_ARG.get(sw, 0)
        if sw == "-I":
            o.setdefault("-I", []).append(argv[k + 1])
        else:
            o[sw] = argv[k + 1:k + 1 + n] if n else True
        k += 1 + n
    if len(argv) - k < 2:
        raise SystemExit(__doc__)
    if "-G" in o and o["-G"][0] != "HTK":
        raise SystemExit("hlstats_bigram: label format %s is not supported (HTK only)" % o["-G"][0])
    if not any(s in o for s in ("-b", "-d", "-l", "-c")):
        raise SystemExit("HLStats: Nothing to do!")
    enter, exit_ = o.get("-s", ["!ENTER", "!EXIT"])
    ls = capi.LabelStats(capi.read_word_list(argv[k]), enter, exit_)
    L = capi.lib()
    loaded = [capi.Mlf(fn) for fn in o.get("-I", [])]            # -I mlf (may be given more than once): where a label file's entries are looked up first
    utts, times = [], []

    def add(handle):
        ids, t = ls.ids_of(handle)
        utts.append(ids)
        times.append(t)

    for fn in argv[k + 1:]:
        if os.path.exists(fn) and open(fn, "rb").read(7) == b"#!MLF!#":      # a master label file among the arguments: every entry of it
            m = capi.Mlf(fn)
            loaded.append(m)
            for _, h in m.entries():
                add(h)
            continue
        lab = os.path.splitext(fn)[0] + "." + o["-X"][0] if "-X" in o else fn      # -X ext, then -L dir, as HLabel's LOpen resolves a name
        if "-L" in o:
            lab = os.path.join(o["-L"][0], os.path.basename(lab))
        found = next((h for h in (L.htkamd_mlf_find(m.h, lab.encode()) for m in loaded) if h), None)
        if found:
            add(found)
            continue
        h = capi.C.c_void_p()
        capi.check(L.htkamd_labels_read(lab.encode(), capi.C.byref(h)), "hlstats_bigram")
        try:
            add(h)
        finally:
            L.htkamd_labels_free(h)
    ls.count(utts, times)
    out = o["--out"][0] if "--out" in o else os.devnull
    open(out, "w").close()
    if "-d" in o:
        ls.stats_write(out, capi.LS_DURS, append=True)
    if "-b" in o:
        ls.bigram_write(o["-b"][0], backoff="-o" in o, uni_floor=float(o.get("-u", [1.0])[0]), big_thresh=int(o.get("-t", [0])[0]), big_floor=float(o.get("-f", [0.0])[0]),
                        discount=float(o.get("--discount", [0.5])[0]), trace_path=o["--trace"][0] if "--trace" in o else None)
    flags = (capi.LS_LIST if "-l" in o else 0) | (capi.LS_COUNTS if "-c" in o else 0)
    if flags:
        ls.stats_write(out, flags, count_limit=int(o.get("-c", [0])[0]), list_path=o.get("-l", [None])[0], append=True)
    print("hlstats_bigram: %d utterances, %d labels, kernels %.3f ms" % (len(utts), sum(len(u) for u in utts), ls.kernel_ms), file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1:])
