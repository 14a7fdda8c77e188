"""What the label-statistics tests share: the committed cases of tests/golden/lm, GatherStats restated in plain Python, and one way to run a
variant of a case through the library."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm")
CASES = sorted(c for c in os.listdir(GOLD) if os.path.isdir(os.path.join(GOLD, c))) if os.path.isdir(GOLD) else []


def load_case(case):
    d = os.path.join(GOLD, case)
    words = open(os.path.join(d, "wordlist")).read().split()
    utts, cur = [], None
    for line in open(os.path.join(d, "labels.mlf")).read().splitlines()[1:]:
        if line.startswith('"'):
            cur = []
        elif line == ".":
            utts.append(cur)
        else:
            s, e, w = line.split()
            cur.append((w, int(s), int(e)))
    return d, words, utts, json.load(open(os.path.join(d, "manifest.json")))


def variants():
    return [(c, v) for c in CASES for v in sorted(load_case(c)[3])]


def boundary(spec):
    sw = spec["hlstats"] or []
    return (sw[sw.index("-s") + 1], sw[sw.index("-s") + 2]) if "-s" in sw else ("!ENTER", "!EXIT")


def gather(id_utts, V, enter, exit_, times=None):
    """GatherStats (HLStats.c:471) over id lists: loop counts per word, the bigram table {(pred, word): n}, durations per word."""
    count, pairs, durs = np.zeros(V, np.int64), {}, {}
    for u, ids in enumerate(id_utts):
        ids = list(ids)
        st, en = 0, len(ids)
        if ids and ids[0] == enter:
            st += 1
        if ids and ids[-1] == exit_:
            en -= 1
        prev = enter
        for p in range(st, en):
            w = ids[p]
            count[w] += 1
            if times is not None:
                durs.setdefault(w, []).append(int(times[u][p][1]) - int(times[u][p][0]))
            if w != enter and w != exit_:
                pairs[(prev, w)] = pairs.get((prev, w), 0) + 1
                prev = w
        pairs[(prev, exit_)] = pairs.get((prev, exit_), 0) + 1
    return count, pairs, durs


def csr(pairs, V):
    """rowOff [V + 1], succ, cnt of a {(pred, word): n} table, as numpy.unique orders the pairs."""
    if not pairs:
        return np.zeros(V + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    keys = np.array(sorted(pairs), np.int64)
    flat, n = np.unique(keys[:, 0] * V + keys[:, 1], return_counts=True)
    assert (n == 1).all()
    rowOff = np.concatenate([[0], np.cumsum(np.bincount(keys[:, 0], minlength=V))]).astype(np.int32)
    return rowOff, (flat % V).astype(np.int32), np.array([pairs[tuple(k)] for k in keys], np.int32)


def case_ids(ls, utts):
    return [np.array([ls.id(w) for w, _, _ in u], np.int32) for u in utts], [np.array([[s, e] for _, s, e in u], np.int64).reshape(-1, 2) for u in utts]


def run_variant(capi, ls, spec, tmp, name):
    """The files HLStats makes for the variant's switches, from a LabelStats that holds counts: {suffix: bytes}."""
    sw = spec["hlstats"]
    opt = lambda k, d: type(d)(sw[sw.index(k) + 1]) if k in sw else d
    out, big, lst = os.path.join(tmp, name + ".out"), os.path.join(tmp, name + ".bigram"), os.path.join(tmp, name + ".list")
    open(out, "w").close()
    if "-d" in sw:
        ls.stats_write(out, capi.LS_DURS)
    ls.bigram_write(big, backoff="-o" in sw, uni_floor=opt("-u", 1.0), big_thresh=opt("-t", 0), big_floor=opt("-f", 0.0),
                    discount=spec["discount"] if spec["discount"] is not None else 0.5, trace_path=out)
    flags = (capi.LS_LIST if "-l" in sw else 0) | (capi.LS_COUNTS if "-c" in sw else 0)
    if flags:
        ls.stats_write(out, flags, count_limit=opt("-c", 0), list_path=lst, append=True)
    got = {"bigram": open(big, "rb").read(), "out": open(out, "rb").read()}
    if "-l" in sw:
        got["list"] = open(lst, "rb").read()
    return got


def build_net(capi, d, words, name, spec, tmp):
    """The variant's network through the library, from the REFERENCE's bigram file: (Network, bytes of its SLF)."""
    hb = spec["hbuild"]
    if "-n" in hb or "-m" in hb:
        enter, exit_ = (hb[hb.index("-s") + 1], hb[hb.index("-s") + 2]) if "-s" in hb else ("!ENTER", "!EXIT")
        lm = capi.Bigram(os.path.join(d, name + ".bigram"))
        net = capi.Network.from_bigram(lm, words + [enter, exit_], enter=enter, exit=exit_)
    else:
        net = capi.Network.word_loop(words, bracket=(hb[1], hb[2]) if "-t" in hb else None)
    path = os.path.join(tmp, name + ".slf")
    net.write(path)
    return net, open(path, "rb").read()
