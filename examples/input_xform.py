#!/usr/bin/env python3
"""A global linear input transform applied to parameter files on the device: the job of `HCopy` with `MATTRANFN = file` set.

    python examples/input_xform.py --xform file --kind MFCC_E_D_A [-d outdir] [--ext htk] files...

Reads the transform file (a `~j "name"` macro file: `<MMFIDMASK> mask <kind> [<PREQUAL>] <LINXFORM> ...`, text or binary), checks it
against the files' kind and --kind (TARGETKIND) as the reference does where it applies a transform, and runs the whole qualifier step in
ONE call in the reference's order (capi.InputXForm.apply = htkamd_inputxform_apply): without <PREQUAL> the qualifiers _D _A _T _Z first
and the matrix over the whole row, with <PREQUAL> the matrix over the statics first and the qualifiers on its outputs.  Every file is
written to outdir under its own name (extension --ext) as an HTK parameter file of --kind, whose rows are as wide as the transform makes
them -- the values HCopy writes, bit for bit.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from htk_amd import capi  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--xform", required=True, help="transform file (what MATTRANFN names)")
    ap.add_argument("--kind", required=True, help="TARGETKIND, e.g. MFCC_E_D_A")
    ap.add_argument("-d", dest="outdir", default=".", help="output directory")
    ap.add_argument("--ext", default="htk", help="extension of the files written")
    ap.add_argument("files", nargs="+")
    a = ap.parse_args(argv)
    xf = capi.InputXForm.read(a.xform)
    stat, per, fileKind = [], 100000, None
    for f in a.files:
        x, per, k = capi.parm_read(f)
        if fileKind not in (None, k) or (stat and x.shape[1] != stat[0].shape[1]):
            sys.exit("%s: kind or width differs from the first file's" % f)
        fileKind = k
        stat.append(x)
    nStat = stat[0].shape[1]
    xf.check_against(capi.parm_kind_str(fileKind), a.kind, nStat)
    dX, frameOff, cols = xf.apply(stat, capi.parm_quals_from_kind(a.kind, nStat))
    rows = dX.to_host(np.float32, (int(frameOff[-1]), cols))
    os.makedirs(a.outdir, exist_ok=True)
    out = []
    for u, f in enumerate(a.files):
        p = os.path.join(a.outdir, os.path.splitext(os.path.basename(f))[0] + "." + a.ext)
        capi.parm_write(p, rows[frameOff[u]:frameOff[u + 1]], per, capi.parm_kind_parse(a.kind))
        out.append(p)
    print("%s (%d x %d%s): %d files, %d frames -> %d columns" % (xf.name, xf.rows, xf.cols, ", <PREQUAL>" if xf.prequal else "", len(out), int(frameOff[-1]), cols))
    return out


if __name__ == "__main__":
    main()
