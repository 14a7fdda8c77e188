"""HQuant: a VQ codebook from parameter files, the clustering on the device.

    python examples/hquant_codebook.py [-d | -f] [-g] [-n S N]... [-s N] [-t] [-F HTK] vqFile trainFiles...

-d / -f: Mahalanobis distance with the pool's diagonal / full covariance (else Euclidean); -g: that global covariance in every node;
-n S N: N entries for stream S (default 256); -s N: streams (the parameter kind's standard split into consecutive columns); -t: tree.
The switches about label segments (-l with -G -I -L -X), -w and -H are refused by name (htkamd_hquant_check_switch).
The pool's mean and covariance (SequenceMean / SequenceCov, HTrain.c:306, :328) are summed here in the reference's order.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htk_amd import capi  # noqa: E402

HASENERGY, HASDELTA, HASACCS, HASZEROC = 0o100, 0o400, 0o1000, 0o20000


def seqsum64(a, chunk=65536):
    """The float64 sum down axis 0 in row order."""
    s = np.zeros(a.shape[1:], np.float64)
    for i in range(0, len(a), chunk):
        s = np.add.accumulate(np.concatenate([s[None], a[i:i + chunk].astype(np.float64)]), axis=0)[-1]
    return s


def sequence_cov(X, kind):
    """SequenceMean, then SequenceCov of `kind` about it: None, the (inverse) variances, or the inverse's packed lower triangle."""
    n, D = np.float64(len(X)), X.shape[1]
    mean = (seqsum64(X) / n).astype(np.float32)
    if kind == capi.CK_NULLC:
        return None
    x = X - mean                                       # float differences
    if kind != capi.CK_FULLC:
        sq = seqsum64(x.astype(np.float64) ** 2)
        return (sq / n if kind == capi.CK_DIAGC else n / sq).astype(np.float32)
    x = x.astype(np.float64)
    t = np.array([seqsum64((x[:, j] * x[:, k])[:, None])[0] / n for j in range(D) for k in range(j + 1)]).astype(np.float32)
    inv = np.zeros_like(t)
    capi.check(capi.lib().htkamd_vq_cov_invert(D, capi._p(t), capi._p(inv)), "vq_cov_invert")
    return inv


def stream_widths(kind, D, S):
    """SetStreamWidths (HParm.c:3094) where the streams are consecutive columns: one stream, or static + deltas (+ accelerations)."""
    if S == 1:
        return [D]
    if kind & (HASENERGY | HASZEROC):
        raise SystemExit("HQuant: -s %d: a kind with a separate energy stream is not split here" % S)
    if S == 2 and (kind & HASDELTA) and not (kind & HASACCS):
        return [D // 2, D // 2]
    if S == 3 and (kind & HASACCS):
        return [D // 3] * 3
    raise SystemExit("HQuant: SetStreamWidths: cant split kind %d into %d streams" % (kind, S))


def main(argv):
    ck, glob, tree, S, sizes, i = capi.CK_NULLC, False, False, 1, {}, 0
    while i < len(argv) and argv[i].startswith("-"):
        sw = argv[i]
        try:
            capi.hquant_check_switch(sw)
        except capi.HtkAmdError as e:
            raise SystemExit(str(e))
        if sw in ("-d", "-f"):
            if ck != capi.CK_NULLC:
                raise SystemExit("HQuant: Specify one of -d or -f, not both")
            ck = capi.CK_INVDIAGC if sw == "-d" else capi.CK_FULLC
        elif sw == "-g":
            glob = True
        elif sw == "-t":
            tree = True
        elif sw == "-n":
            sizes[int(argv[i + 1])] = int(argv[i + 2]); i += 2
        elif sw == "-s":
            S = int(argv[i + 1]); i += 1
        elif sw == "-F":
            if argv[i + 1] != "HTK":
                raise SystemExit("HQuant: -F %s: only HTK parameter files are read" % argv[i + 1])
            i += 1
        i += 1
    if len(argv) - i < 2:
        raise SystemExit(__doc__)
    out, files = argv[i], argv[i + 1:]
    data, kind0 = [], None
    for f in files:
        X, _, kind = capi.parm_read(f)[:3]
        if kind0 is not None and (kind != kind0 or X.shape[1] != data[0].shape[1]):
            raise SystemExit("HQuant: CheckData: %s differs from data already read" % f)
        kind0 = kind
        data.append(X)
    X = np.concatenate(data)
    widths = stream_widths(kind0, X.shape[1], S)
    sets, gcov, col = [], [], 0
    for s, D in enumerate(widths):
        Xs = np.ascontiguousarray(X[:, col:col + D])
        col += D
        cov = sequence_cov(Xs, ck)
        dX = capi.DevArray(Xs)
        sets.append(capi.vq_cluster(dX.ptr, len(Xs), D, sizes.get(s + 1, 256), tree=tree, dist_kind=ck, dist_cov=cov))
        dX.free()
        gcov.append(cov if glob else None)
    capi.VQ(clusters=sets, kind=ck, magic=kind0, global_cov=gcov).write(out)
    return sets


if __name__ == "__main__":
    main(sys.argv[1:])
