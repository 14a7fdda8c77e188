"""Fixtures of tests/golden/lm: word lists and label MLFs of our own, and what the reference's HLStats and HBuild make of them.

    make -C oracle _ref/HLStats _ref/HBuild && python tests/golden/make_lm_golden.py

Only the tools' inputs and outputs are kept.  Per case: wordlist, labels.mlf, manifest.json (the variants with their switches), and per
variant NAME.bigram / NAME.out (standard output) / NAME.list / NAME.slf as far as the variant makes them.

The reference's word loop lists its words in the order of its vocabulary's hash table, whose slots are the ADDRESSES of the names modulo
701: the order differs between runs of the same command.  For the four-word case the generator repeats HBuild until the words come out
in word-list order, which is the order the library defines; larger lists never do.
"""
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, "..", "..", "oracle", "_ref")
OUT = os.path.join(HERE, "lm")

# name -> (HLStats switches, DISCOUNT or None, HBuild switches or None)
VARIANTS = {
    "bo": (["-o"], None, ["-n"]),
    "bo_t1_u05": (["-o", "-t", "1", "-u", "0.5"], None, ["-n"]),
    "bo_disc03": (["-o"], 0.3, None),
    "mat": ([], None, ["-m"]),
    "mat_f001": (["-f", "0.01"], None, ["-m"]),
    "bo_sent": (["-o", "-s", "SENT-START", "SENT-END"], None, ["-s", "SENT-START", "SENT-END", "-n"]),
    "lists": (["-o", "-c", "5", "-d", "-l", "@LIST"], None, None),
}


def toy():
    words = ["a", "b", "c", "d"]
    utts = [[("a", 0, 300000), ("b", 300000, 500000), ("a", 500000, 900000)],
            [("c", 0, 100000), ("a", 100000, 500000), ("b", 500000, 700000), ("zz", 700000, 900000)],      # zz: not in the list
            [("b", 0, 100000)],
            [("!ENTER", 0, 100000), ("a", 100000, 300000), ("!EXIT", 300000, 400000)]]
    return words, utts


def rand_case(seed, V, n_utt, max_len):
    rng = random.Random(seed)
    words = sorted({"w%s" % "".join(rng.choice("abcdefgh") for _ in range(rng.randint(1, 3))) for _ in range(V * 3)})[:V]
    rng.shuffle(words)
    weights = [1.0 / (k + 1) for k in range(len(words))]
    weights[-1] = 0.0                                         # a word that never occurs: it has no successors
    utts = []
    for _ in range(n_utt):
        t, u = 0, []
        for w in rng.choices(words, weights, k=rng.randint(1, max_len)):
            d = rng.randint(1, 9) * 100000
            u.append((w, t, t + d))
            t += d
        utts.append(u)
    for u in utts[:5]:                                        # the last word seen only at the end of utterances: a row with !EXIT alone
        u.append((words[-2], u[-1][2], u[-1][2] + 100000))
    return words, utts


def decode_case():
    """The words of tests/golden/decode/bigram's dictionary: the model behind the network of tests/test_gpu_netbuild_decode.py."""
    words = ["AB", "CD", "E", "F", "G", "H", "I"]
    rng = random.Random(3)
    return words, [[(w, 100000 * k, 100000 * (k + 1)) for k, w in enumerate(rng.choices(words, [4, 3, 1, 1, 2, 2, 3], k=rng.randint(1, 6)))] for _ in range(40)]


# every variant on the two small cases; the 200-word case keeps the one variant whose files stay short (-t 1 drops the singleton bigrams)
CASES = {"toy": toy(), "rand12": rand_case(7, 12, 50, 8), "rand200": rand_case(11, 200, 80, 10), "decode7": decode_case()}
ONLY = {"rand200": ("bo_t1_u05",), "decode7": ("bo",)}


def run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw)
    if r.returncode:
        sys.exit("%s\n%s" % (" ".join(cmd), r.stderr.decode()))
    return r.stdout


def slf_words(path):
    return [l.split("W=")[1].split()[0] for l in open(path) if l.startswith("I=")]


def main():
    for case, (words, utts) in CASES.items():
        d = os.path.join(OUT, case)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "wordlist"), "w") as f:
            f.write("".join(w + "\n" for w in words))
        with open(os.path.join(d, "labels.mlf"), "w") as f:
            f.write("#!MLF!#\n")
            for k, u in enumerate(utts):
                f.write('"*/u%03d.lab"\n' % k + "".join("%d %d %s\n" % (s, e, w) for w, s, e in u) + ".\n")
        manifest = {}
        for name, (sw, disc, hb) in VARIANTS.items():
            if name not in ONLY.get(case, VARIANTS):
                continue
            cfg = os.path.join(d, "_cfg")
            with open(cfg, "w") as f:
                f.write("DISCOUNT = %s\n" % disc if disc is not None else "")
            big, lst = os.path.join(d, name + ".bigram"), os.path.join(d, name + ".list")
            sw2 = [lst if x == "@LIST" else x for x in sw]
            out = run([os.path.join(REF, "HLStats"), "-C", cfg, "-T", "4", "-b", big] + sw2 + [os.path.join(d, "wordlist"), os.path.join(d, "labels.mlf")])
            os.remove(cfg)
            with open(os.path.join(d, name + ".out"), "wb") as f:
                f.write(out)
            manifest[name] = dict(hlstats=sw, discount=disc, hbuild=hb)
            if hb is not None:
                enter, exit_ = (sw[sw.index("-s") + 1], sw[sw.index("-s") + 2]) if "-s" in sw else ("!ENTER", "!EXIT")
                wl = os.path.join(d, "_hbuild_words")
                with open(wl, "w") as f:
                    f.write("".join(w + "\n" for w in words + [enter, exit_]))
                run([os.path.join(REF, "HBuild")] + hb + [big, wl, os.path.join(d, name + ".slf")])
                os.remove(wl)
        for name, hb in (("loop", []), ("loop_t", ["-t", "!ENTER", "!EXIT"])) if case == "toy" else ():
            slf = os.path.join(d, name + ".slf")
            for _ in range(200):
                run([os.path.join(REF, "HBuild")] + hb + [os.path.join(d, "wordlist"), slf])
                if [w for w in slf_words(slf) if w not in ("!NULL", "!ENTER", "!EXIT")] == words:
                    break
            else:
                os.remove(slf)
                print("%s/%s: the reference never gave the word-list order; no fixture" % (case, name))
                continue
            manifest[name] = dict(hlstats=None, discount=None, hbuild=hb)
        with open(os.path.join(d, "manifest.json"), "w") as f:
            json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
