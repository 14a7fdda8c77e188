"""A plain restatement of what HLRescore computes on a lattice (HLat.c: LatTopSort :423, LatFindBest :575, LatForwBackw :490 with LATFB_MAX,
LatPrune :711), for the tests of htk_amd's lattice set: the node order, the two orders in which the loops meet arcs, and the three recursions.
LArcTotLike (HNet.h:257) is numpy.float32 arithmetic plus a double word penalty; everything else is fp64 in the reference's order.
test_latrescore_host.py pins this file to the reference's recorded outputs; the GPU tests then use it where no fixture exists."""
import gzip
import json
import os

import numpy as np

LZERO = -1.0e10
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "latrescore")
NBIN = 1000

_fix = None


def fixtures():
    """The generator's record (tests/golden/make_latrescore_golden.py), read once."""
    global _fix
    if _fix is None:
        _fix = json.loads(gzip.open(os.path.join(GOLD, "fixtures.json.gz"), "rt").read())
    return _fix


def unpack_group(name, into):
    """Writes a group's dictionary and lattices under `into`; returns (dict path, {lattice name: path})."""
    g = fixtures()["groups"][name]
    os.makedirs(into, exist_ok=True)
    dpath = os.path.join(into, "dict")
    open(dpath, "w").write(g["dict"])
    lats = {}
    for n, t in g["lats"].items():
        if isinstance(t, dict):
            lats[n] = os.path.join(ROOT, t["path"])
        else:
            lats[n] = os.path.join(into, n + ".lat")
            open(lats[n], "w").write(t)
    return dpath, lats


def setting_of(args):
    """(a, s, p, r) of a run's switches, HLRescore's defaults elsewhere."""
    v = dict(a=1.0, s=1.0, p=0.0, r=1.0)
    for i, x in enumerate(args):
        if x in ("-a", "-s", "-p", "-r"):
            v[x[1]] = float(args[i + 1])
    return (v["a"], v["s"], v["p"], v["r"])


def read_dict(path):
    """word -> [(pnum, outSym or None)] for dictionaries as plain as the fixtures'."""
    d = {}
    for line in open(path):
        tok = line.split()
        if not tok:
            continue
        out = tok[0]
        if len(tok) > 1 and tok[1].startswith("[") and tok[1].endswith("]"):
            out = tok[1][1:-1] or None
        d.setdefault(tok[0], []).append((len(d.get(tok[0], [])) + 1, out))
    return d


def read_slf(path):
    """One level of SLF text, fields separated by blanks, no quoting (the fixtures have none)."""
    nn = na = None
    lat = None
    for line in open(path):
        f = dict(x.split("=", 1) for x in line.split() if "=" in x and not x.startswith("#"))
        if lat is None:
            if "N" in f and "L" in f:
                nn, na = int(f["N"]), int(f["L"])
                lat = dict(nNodes=nn, nArcs=na, nodeTime=np.zeros(nn), word=["!NULL"] * nn, var=[-1] * nn, arcStart=np.zeros(na, np.int64),
                           arcEnd=np.zeros(na, np.int64), arcAc=np.zeros(na, np.float32), arcLm=np.zeros(na, np.float32), arcPr=np.zeros(na, np.float32), line=[])
            continue
        if line.startswith("I="):
            i = int(f["I"])
            lat["nodeTime"][i] = float(f.get("t", 0.0)); lat["word"][i] = f.get("W", "!NULL"); lat["var"][i] = int(f.get("v", -1))
        elif line.startswith("J="):
            j = int(f["J"])
            lat["arcStart"][j], lat["arcEnd"][j] = int(f["S"]), int(f["E"])
            lat["arcAc"][j], lat["arcLm"][j], lat["arcPr"][j] = float(f.get("a", 0.0)), float(f.get("l", 0.0)), float(f.get("r", 0.0))
            lat["line"].append(j)
    lat["nullEnd"] = np.array([lat["word"][e] == "!NULL" for e in lat["arcEnd"]], bool)
    return lat


def from_view(v):
    """A lattice of capi.LatSet.view with arcs taken in number order (lattices made by add / add_pruned)."""
    lat = dict(v)
    lat["line"] = list(range(v["nArcs"]))
    return lat


def orders(lat):
    """start, end, LatTopSort's order, and the arcs as the forward and the backward loop meet them.  An arc joins the FRONT of its nodes'
    lists as its line is read (HNet.c:1189-1192)."""
    nn = lat["nNodes"]
    foll, pred = [[] for _ in range(nn)], [[] for _ in range(nn)]
    for a in lat["line"]:
        foll[lat["arcStart"][a]].insert(0, a); pred[lat["arcEnd"][a]].insert(0, a)
    start = next(i for i in range(nn) if not pred[i])
    end = next(i for i in range(nn) if not foll[i])
    num, time = [-1] * nn, -1
    stack = [(end, iter(pred[end]))]
    num[end] = -2
    while stack:
        n, it = stack[-1]
        a = next(it, None)
        if a is None:
            time += 1; num[n] = time; stack.pop(); continue
        s = int(lat["arcStart"][a])
        if num[s] == -1:
            num[s] = -2; stack.append((s, iter(pred[s])))
    assert time + 1 == nn
    top = [0] * nn
    for i, t in enumerate(num):
        top[t] = i
    fwd = [a for n in top for a in foll[n]]
    bwd = [a for n in reversed(top) for a in pred[n]]
    return dict(start=start, end=end, top=np.array(top), fwd=np.array(fwd, np.int64), bwd=np.array(bwd, np.int64))


def tot_like(lat, setting):
    """LArcTotLike per arc, as a double."""
    a, s, p, r = [np.float32(x) for x in setting]
    f = (lat["arcAc"].astype(np.float32) * a + lat["arcLm"].astype(np.float32) * s) + lat["arcPr"].astype(np.float32) * r
    assert f.dtype == np.float32
    return f.astype(np.float64) + np.where(lat["nullEnd"], 0.0, np.float64(p))


def find_best(lat, o, setting):
    like = tot_like(lat, setting)
    score, back = np.full(lat["nNodes"], LZERO), [-1] * lat["nNodes"]
    score[o["start"]] = 0.0
    S, E = lat["arcStart"], lat["arcEnd"]
    for a in o["fwd"]:
        v = score[S[a]] + like[a]
        if v > score[E[a]]:
            score[E[a]] = v; back[E[a]] = int(a)
    path, n = [], o["end"]
    ac = lm = pr = tot = 0.0
    while back[n] >= 0:
        a = back[n]
        path.append(a)
        ac += float(lat["arcAc"][a]); lm += float(lat["arcLm"][a]); pr += float(lat["arcPr"][a]); tot += float(like[a])
        n = int(S[a])
    return np.array(path[::-1], np.int32), np.array([ac, lm, pr, tot])


def fb_max(lat, o, setting):
    like = tot_like(lat, setting)
    fw, bw = np.full(lat["nNodes"], LZERO), np.full(lat["nNodes"], LZERO)
    fw[o["start"]] = 0.0; bw[o["end"]] = 0.0
    S, E = lat["arcStart"], lat["arcEnd"]
    for a in o["fwd"]:
        v = fw[S[a]] + like[a]
        if v > fw[E[a]]:
            fw[E[a]] = v
    for a in o["bwd"]:
        v = bw[E[a]] + like[a]
        if v > bw[S[a]]:
            bw[S[a]] = v
    return fw, bw, bw[o["top"][0]]


def prune(lat, o, setting, thresh, arcs_per_sec=0.0):
    """LatPrune's keep flags (beamPruneArcs = T)."""
    like = tot_like(lat, setting)
    fw, bw, best = fb_max(lat, o, setting)
    thresh = float(thresh)
    limit = best - thresh
    S, E = lat["arcStart"], lat["arcEnd"]
    arc = (fw[S] + like) + bw[E]
    aps = np.float32(arcs_per_sec)
    if aps > 0:
        n_limit = int(float(lat["nodeTime"][o["end"]]) * float(aps))
        width = np.float32(thresh / NBIN)
        hist = [0] * NBIN
        n = 0
        for sc in arc:
            q = (best - sc) / float(width)
            if q < NBIN:
                hist[int(q)] += 1; n += 1
        if n > n_limit:
            n = 0
            for i in range(NBIN):
                n += hist[i]
                if n > n_limit:
                    break
            thresh = float(np.float32(i) * width)
            limit = best - thresh
    return (fw + bw) >= limit, arc >= limit


def compact(lat, keep_node, keep_arc):
    """LatPrune's new lattice: survivors in their order, renumbered; the new lists are filled in arc order."""
    renum = np.cumsum(keep_node) - 1
    ka = np.flatnonzero(keep_arc)
    out = dict(nNodes=int(keep_node.sum()), nArcs=len(ka), nodeTime=lat["nodeTime"][keep_node], arcStart=renum[lat["arcStart"][ka]], arcEnd=renum[lat["arcEnd"][ka]],
               arcAc=lat["arcAc"][ka], arcLm=lat["arcLm"][ka], arcPr=lat["arcPr"][ka], nullEnd=lat["nullEnd"][ka], line=list(range(len(ka))))
    if "word" in lat:
        out["word"] = [w for w, k in zip(lat["word"], keep_node) if k]; out["var"] = [v for v, k in zip(lat["var"], keep_node) if k]
    return out


def labels(lat, dic, setting, path):
    """LatFindBest's label list: (start, end, name, float score)."""
    like = tot_like(lat, setting)
    out = []
    for a in path:
        e = int(lat["arcEnd"][a])
        w = lat["word"][e]
        if w == "!NULL":
            continue
        name = next((o for n, o in dic.get(w, []) if n == lat["var"][e]), w)
        if name is None:
            continue
        out.append((lat["nodeTime"][int(lat["arcStart"][a])] * 1.0e7, lat["nodeTime"][e] * 1.0e7, name, np.float32(like[a])))
    return out
