"""HCompV for a prototype with full covariances: the flat start of a <FULLC> set, the statistics on the device's fp64 matrix pipe.

    python examples/hcompv_fullc.py [-m] [-f F] [-v V] [-l LAB] [-L DIR] [-I MLF] [-M DIR] [-S SCP] proto [trainFiles...]

-m: update the means too; -f F: write vFloors with F times the global variance; -v V: floor of the variances (the diagonal);
-l LAB: only the segments labelled LAB (label files from -L DIR or the master label file -I MLF), else the whole files; -M DIR: where
the set and vFloors go (default: beside the prototype's name in the current directory); -S SCP: a script of parameter files.

The parameter files are uploaded as one table; -l becomes the segment list (a label's frames are start / period .. end / period,
the end clipped to the file, LoadFile HCompV.c:463-471); htkamd_compv_full gives count, sum and the triangle of squares in one call;
htkamd_compv_full_cov turns them into mean, covariance and inverse covariance (CalcCovs :261-297).  A FULLC prototype gets the inverse
covariance in every mixture, a DIAGC one the covariance's diagonal (SetCovs :345-352).  A prototype of several streams is refused.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htk_amd import capi  # noqa: E402


def label_frames(labels, seg_label, period, n_frames):
    """The (first, count) of every case of seg_label: LoadFile's segStIdx .. segEnIdx, the end clipped to the file."""
    out = []
    for name, start, end, _ in labels:
        if name == seg_label:
            a, e = int(start / period), min(int(end / period), n_frames - 1)
            if e >= a:
                out.append((a, e - a + 1))
    return out


def main(argv):
    opt = {"-m": False, "-f": None, "-v": 0.0, "-l": None, "-L": None, "-I": None, "-M": None, "-S": None}
    i = 0
    while i < len(argv) and argv[i].startswith("-"):
        sw = argv[i]
        if sw not in opt:
            raise SystemExit("HCompV: switch %s is not served here (-m -f -v -l -L -I -M -S are)" % sw)
        if sw == "-m":
            opt[sw] = True
        else:
            opt[sw] = float(argv[i + 1]) if sw in ("-f", "-v") else argv[i + 1]
            i += 1
        i += 1
    if i >= len(argv):
        raise SystemExit(__doc__)
    proto, files = argv[i], argv[i + 1:] + ([phys for _, phys, _, _ in capi.scp_read(opt["-S"])] if opt["-S"] else [])
    mmf = capi.Mmf(files=[proto])
    if mmf.desc.numStreams > 1:
        raise SystemExit("HCompV: %s has %d streams; only a one-stream prototype is served" % (proto, mmf.desc.numStreams))
    mmf.refuse_input_xform("hcompv_fullc")
    pk = mmf.packed()
    D = pk["vecSize"]
    mlf = capi.Mlf(opt["-I"]) if opt["-I"] else None
    data, segs, base = [], [], 0
    for f in files:
        X, period, _ = capi.parm_read(f)
        if X.shape[1] != D:
            raise SystemExit("HCompV: CheckData: Vector size in %s[%d] is incompatible with hmm %s[%d]" % (f, X.shape[1], proto, D))
        if opt["-l"] is None:
            segs.append((base, len(X), 0))
        else:
            stem = os.path.splitext(os.path.basename(f))[0]
            labels = mlf.find(f) if mlf else capi.labels_read(os.path.join(opt["-L"] or os.path.dirname(f), stem + ".lab"))
            segs += [(base + a, n, 0) for a, n in label_frames(labels or [], opt["-l"], period, len(X))]
        data.append(X)
        base += len(X)
    if not data:
        raise SystemExit("HCompV: no training files")
    dX = capi.DevArray(np.concatenate(data))
    count, s, q = capi.compv_full(dX.ptr, base, D, segs=segs, nClass=1)      # the one library call over all files
    dX.free()
    full = mmf.cov_kind == "FULLC"
    try:
        mean, cov, inv = capi.compv_full_cov(count[0], s[0], q[0], minVar=opt["-v"], want_inverse=full)
    except capi.HtkAmdError as e:
        raise SystemExit("HCompV: " + str(e))
    diag = cov[[x * (x + 1) // 2 + x for x in range(D)]]
    G = pk["numGauss"]
    if opt["-m"]:
        pk["mean"] = np.tile(mean, (G, 1))
    if full:                                           # <GCONST> as FixFullGConst (HModel.c:5682) and FixDiagGConst (:5641) leave it
        pk["invCov"] = np.tile(inv, (G, 1))
        m = np.zeros((D, D))
        m[np.tril_indices(D)] = inv
        gconst = D * np.log(2.0 * np.pi) - np.linalg.slogdet(m + np.tril(m, -1).T)[1]
    else:
        pk["var"] = np.tile(diag, (G, 1))
        gconst = D * np.log(2.0 * np.pi) + np.log(diag.astype(np.float64)).sum()
    pk["gconst"] = np.full(G, gconst, np.float32)
    out_dir = opt["-M"] or "."
    mmf.write(pk, out_dir=out_dir)
    if opt["-f"] is not None:
        capi.write_vfloors(os.path.join(out_dir, "vFloors"), diag, opt["-f"])      # PutVFloor :374-379: the covariance's diagonal
    return count[0], mean, cov, inv


if __name__ == "__main__":
    main(sys.argv[1:])
