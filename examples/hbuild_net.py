"""HBuild on the device: a word loop, or the network of a back-off or matrix bigram, written as the SLF file the reference writes.

    python examples/hbuild_net.py [-n bigram | -m bigram] [-s s1 s2] [-t s1 s2] [-u s] [-z] wordList latFile

The switches are HBuild's own.  -x, -w, -L, -j and -b are refused by name."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htk_amd import capi

WITH_ARG = {"-n": 1, "-m": 1, "-s": 2, "-t": 2, "-u": 1}


def main(argv):
    o, k = {}, 0
    while k < len(argv) and argv[k].startswith("-") and len(argv[k]) > 1:
        sw = argv[k]
        capi.check(capi.lib().htkamd_netbuild_check_switch(sw.encode()), "hbuild_net")
        n = WITH_ARG.get(sw, 0)
        o[sw] = argv[k + 1:k + 1 + n] if n else True
        k += 1 + n
    if len(argv) - k != 2:
        raise SystemExit(__doc__)
    if "-n" in o and "-m" in o:
        raise SystemExit("HBuild: Can only specifiy one of -m, -n, -w, -x")
    words = capi.read_word_list(argv[k])
    if "-n" in o or "-m" in o:
        lm = capi.Bigram((o.get("-n") or o.get("-m"))[0])
        if lm.type != (capi.LM_BACKOFF if "-n" in o else capi.LM_MATRIX):
            raise SystemExit("HBuild: File specified is not a %s bigram" % ("back-off" if "-n" in o else "matrix"))
        enter, exit_ = o.get("-s", ["!ENTER", "!EXIT"])
        net = capi.Network.from_bigram(lm, words, enter=enter, exit=exit_, unknown=o.get("-u", ["!NULL"])[0], zap_unknown="-z" in o)
    else:
        net = capi.Network.word_loop(words, bracket=o.get("-t"))
    net.write(argv[k + 1])


if __name__ == "__main__":
    main(sys.argv[1:])
