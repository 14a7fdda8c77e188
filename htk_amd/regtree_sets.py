"""Synthetic one-stream DIAGC model sets as text, with a statistics file and an `LS stats` + `RC` edit script: what the regression class
tree's fixtures, tests and tools/regtree_bench.py are built from.  Both HHEd and this library read the files; the numbers are written with
%e, so both parse the same floats."""
import os

import numpy as np

IDENT = "rtree"


def _vec(key, v):
    return "<%s> %d\n %s\n" % (key, len(v), " ".join("%e" % x for x in v))


def _pdf(mean, var):
    return _vec("MEAN", mean) + _vec("VARIANCE", var)


def _transp(n):
    a = np.zeros((n, n))
    a[0, 1] = 1.0
    for i in range(1, n - 1):
        a[i, i], a[i, i + 1] = 0.6, 0.4
    return "<TRANSP> %d\n" % n + "".join(" " + " ".join("%e" % x for x in row) + "\n" for row in a)


def write_set(d, names, n_emit, n_mix, D, seed, spread=3.0, occ_zero=(), tied=False, twins=(), dyadic=False, clusters=0):
    """hmmdefs, hmmlist and stats under `d`.  occ_zero: (model index, emitting state index) pairs whose occupation is 0 in the statistics.
    tied: state 3 of the first two models is one ~s macro and mixture 2 of state 2 of the last two models one ~m macro.  twins: pairs of
    (model, state, mix) triples (0-based) that get the same mean.  dyadic: means k/8, symmetric about 0 inside every state (mixture 2 is
    minus mixture 1), mixture weights 0.5, occupations powers of two, and two Gaussians at exactly 0 -- every sum is exact, the root's mean
    is exactly 0 and the Gaussians at 0 are exactly as far from one seed as from the other.  clusters > 0: the means are drawn around that
    many well-separated centres of unequal weight (k-means then needs many iterations to settle)."""
    rng = np.random.RandomState(seed)
    H, S, M = len(names), n_emit, n_mix
    if clusters:
        cen = rng.randn(clusters, D) * spread
        pick = rng.randint(0, clusters, size=(H, S, M))
        mean = cen[pick] + rng.randn(H, S, M, D) * (spread * 0.9)
    else:
        mean = rng.randn(H, S, M, D) * spread
    var = 0.5 + rng.rand(H, S, M, D)
    wt = rng.rand(H, S, M) + 0.2
    wt /= wt.sum(axis=2, keepdims=True)
    occ = 5.0 + 100.0 * rng.rand(H, S)
    if dyadic:
        assert M == 2
        mean = np.round(mean * 8.0) / 8.0
        mean[:, :, 1, :] = -mean[:, :, 0, :]
        mean[0, 0, :, :] = 0.0
        var = np.round(var * 8.0) / 8.0
        var[:, :, 1, :] = var[:, :, 0, :]
        wt[:] = 0.5
        occ = 2.0 ** rng.randint(1, 5, size=(H, S))
    for a, b in twins:
        mean[b] = mean[a]
    for h, s in occ_zero:
        occ[h, s] = 0.0
    out = ["~o\n<STREAMINFO> 1 %d\n<VECSIZE> %d<NULLD><USER><DIAGC>\n" % (D, D)]
    if tied:
        out.append('~s "shared_s"\n<NUMMIXES> %d\n' % M + "".join("<MIXTURE> %d %e\n" % (m + 1, wt[0, 1, m]) + _pdf(mean[0, 1, m], var[0, 1, m]) for m in range(M)))
        out.append('~m "shared_m"\n' + _pdf(mean[H - 1, 0, 1], var[H - 1, 0, 1]))
    for h, name in enumerate(names):
        out.append('~h "%s"\n<BEGINHMM>\n<NUMSTATES> %d\n' % (name, S + 2))
        for s in range(S):
            out.append("<STATE> %d\n" % (s + 2))
            if tied and s == 1 and h < 2:
                out.append('~s "shared_s"\n')
                continue
            out.append("<NUMMIXES> %d\n" % M)
            for m in range(M):
                out.append("<MIXTURE> %d %e\n" % (m + 1, wt[h, s, m]))
                if tied and s == 0 and m == 1 and h >= H - 2:
                    out.append('~m "shared_m"\n')
                else:
                    out.append(_pdf(mean[h, s, m], var[h, s, m]))
        out.append(_transp(S + 2) + "<ENDHMM>\n")
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "hmmdefs"), "w").write("".join(out))
    open(os.path.join(d, "hmmlist"), "w").write("\n".join(names) + "\n")
    open(os.path.join(d, "stats"), "w").write("".join("%5d \"%s\" %4d %s\n" % (h + 1, n, 10 + h, " ".join("%f" % x for x in occ[h])) for h, n in enumerate(names)))


def names_for(n, sil=False):
    base = ["m%02d" % k for k in range(n)]
    return (["sil"] + base[1:]) if sil else base


def write_script(d, n_terminals, items=None, ident=IDENT, name="rc.hed"):
    open(os.path.join(d, name), "w").write("LS stats\nRC %d %s%s\n" % (n_terminals, ident, " " + items if items else ""))
