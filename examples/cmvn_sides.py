#!/usr/bin/env python3
"""Side-based cepstral mean and variance statistics on the device: the job of `HCompV -c dir -k mask [-p mask] -q nmv`.

    python examples/cmvn_sides.py -k '*/%%%_*.mfc' -c cmn [-p '%??'] [-q nmv] [--kind MFCC_E_D_A] [--normalise outdir --varscale file] files...

Every parameter file goes to the side its name gives under the mask -k (% captures a character, ? matches one, * any run).  The files
are coded as --kind (default: as they are; _D _A _T are appended on the device), the per-side sums are taken in ONE call
(capi.side_stats: fp64, deterministic) and every side's `<CEPSNORM> <KIND>` file is written to -c (under the directory level that -p
captures from the side's name, when given) with the lines -q asks for: m, v, mv, nv or nmv.

--normalise outdir: the files are then normalised with what was estimated -- the side's mean subtracted (the kind gains _Z), and with
--varscale file (a `<VARSCALE> n ...` global variance) every column scaled by sqrt(global / side variance) -- and written to outdir
as HTK parameter files: what HCopy writes with CMEANDIR / CMEANMASK (and VARSCALEDIR / VARSCALEMASK / VARSCALEFN) set.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from htk_amd import capi  # noqa: E402

HASZEROM = 0o4000


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-k", dest="mask", required=True, help="side mask (HCompV -k)")
    ap.add_argument("-c", dest="outdir", required=True, help="directory of the side files (HCompV -c)")
    ap.add_argument("-p", dest="pathmask", default=None, help="path mask on the side's name (HCompV -p)")
    ap.add_argument("-q", dest="flags", default="nmv", help="lines to write: m v mv nv nmv (HCompV -q)")
    ap.add_argument("--kind", default=None, help="TARGETKIND the statistics are taken of (default: the files' kind)")
    ap.add_argument("--normalise", default=None, metavar="DIR", help="also write the normalised files here")
    ap.add_argument("--varscale", default=None, help="<VARSCALE> file: with --normalise, scale the variances too")
    ap.add_argument("files", nargs="+")
    a = ap.parse_args()
    if "%" not in a.mask or (a.pathmask and "%" not in a.pathmask):
        sys.exit("a mask without % captures nothing")

    sides, uttSide, stat, per, fileKind = [], [], [], 100000, None
    for f in a.files:
        side = capi.mask_match(a.mask, f)
        if side is None:
            sys.exit("speaker pattern matching failure on file: %s" % f)
        if side not in sides:
            sides.append(side)
        uttSide.append(sides.index(side))
        x, per, k = capi.parm_read(f)
        if fileKind not in (None, k):
            sys.exit("%s: kind differs from the first file's" % f)
        fileKind = k
        stat.append(x)
    kindStr = a.kind or capi.parm_kind_str(fileKind)
    kind = capi.parm_kind_parse(kindStr)
    if kind < 0 or (kind & ~0o105400) != (fileKind & ~0o105400):
        sys.exit("--kind %s cannot be derived from files of kind %s" % (kindStr, capi.parm_kind_str(fileKind)))
    if kind & HASZEROM and "m" in a.flags:
        print("warning: qualifier _Z not appropriate when calculating means", file=sys.stderr)
    if kind == fileKind:
        table = np.concatenate(stat)
        frameOff = capi.offsets([x.shape[0] for x in stat])
        dX, cols = capi.DevArray(table), table.shape[1]
    else:
        dX, frameOff, cols = capi.parm_qualify(stat, capi.parm_quals_from_kind(kindStr, stat[0].shape[1]))
    s, q, n = capi.side_stats(dX.ptr, frameOff, uttSide, len(sides), cols, cols)
    mean, var = capi.side_stats_finish(s, q, n)
    for i, side in enumerate(sides):
        d = a.outdir
        if a.pathmask:
            sub = capi.mask_match(a.pathmask, side)
            if sub is None:
                sys.exit("path pattern matching failure on speaker: %s" % side)
            d = os.path.join(d, sub)
        os.makedirs(d, exist_ok=True)
        capi.cepsnorm_write(os.path.join(d, side), kind, a.flags, int(n[i]), mean[i], var[i])
        print("%s: %d frames in %d files" % (side, n[i], uttSide.count(i)))

    if a.normalise:
        if kind & HASZEROM:
            sys.exit("--normalise: the files are zero-meaned per utterance already (_Z)")
        scale = capi.cepsnorm_scale(capi.varscale_read(a.varscale), var, sides) if a.varscale else None
        capi.parm_normalise(dX.ptr, frameOff, uttSide, len(sides), cols, mean=mean, scale=scale)
        out = dX.to_host(np.float32, (int(frameOff[-1]), cols))
        os.makedirs(a.normalise, exist_ok=True)
        for u, f in enumerate(a.files):
            capi.parm_write(os.path.join(a.normalise, os.path.basename(f)), out[frameOff[u]:frameOff[u + 1]], per, kind | HASZEROM)


if __name__ == "__main__":
    main()
