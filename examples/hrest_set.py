#!/usr/bin/env python3
"""HRest for EVERY model of a list in one call (htkamd_hrest) -- the data flow of, for each model X of the list,
    HRest -C cfg -S scp -L labdir|-I mlf -l X -i n -e f -v f -m n -w f -u tmvw [-t] -T 1 -M outdir srcdir/X
with every model's tokens taken from its own labels (one label per model; -l with a label shared by several models is not served).
All models go into one library call: per pass one forward-backward batch over the tokens of the models still running, the sums of
the log probabilities and the updates on the device.  Example with the HTKDemo fixtures of this repository:

    python examples/hrest_set.py --hmmlist tests/golden/demo/bcplist --hmmdir tests/golden/demo/hmm0 \
        --data tests/golden/demo/train/*.mfc --labdir tests/golden/demo/labels --target-kind MFCC_E_D -i 10 -v 0.05 -w 3 -o /tmp/hmm1
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from htk_amd import capi  # noqa: E402
from examples.hinit_set import tokens_from_labels, uflags_of  # noqa: E402

STATUS_TEXT = {capi.HREST_EFEWSEGS: "Too Few Training Examples", capi.HREST_EZEROOCC: "Zero occupation count",
               capi.HREST_EFLOORSUM: "FloorMixes: Floor sum too large", capi.HREST_ENOUSABLE: "ReEstimateModel: No Usable Training Examples"}


def trace_lines(name, r):
    """what the reference prints under -T 1 for one model (ReEstimateModel HRest.c:1340-1355), each line behind 'HRest <name>: '"""
    out, old = [], None
    for k, (p, n) in enumerate(zip(r["logP"], r["used"])):
        line = "Ave LogProb at iter %d = %10.5f using %d examples" % (k + 1, p, n)
        if k > 0:
            line += "  change = %10.5f" % float(np.float32(p) - np.float32(old))
        out.append(line); old = p
    if r["status"] != capi.HREST_OK:
        out.append("ERROR [+%d] %s: the model is written as it came" % (r["status"], STATUS_TEXT.get(r["status"], "")))
    else:
        out.append("Estimation %s at iteration %d" % ("converged" if r["converged"] else "aborted", r["passes"]))
    return ["HRest %s: %s" % (name, l) for l in out]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hmmlist", required=True)
    ap.add_argument("--mmf", action="append", default=[], help="master macro file(s) with the models to re-estimate")
    ap.add_argument("--hmmdir", help="directory with one file per model")
    ap.add_argument("--scp", help="script file: one parameter file per line (HRest -S)")
    ap.add_argument("--data", nargs="*", default=[], help="parameter files")
    ap.add_argument("--labdir", help="directory of label files (HRest -L)")
    ap.add_argument("--mlf", help="master label file (HRest -I)")
    ap.add_argument("--target-kind", default=None, help="e.g. MFCC_E_D: qualifiers _D/_A missing in the files are computed (TARGETKIND)")
    ap.add_argument("-i", "--maxiter", type=int, default=20, help="HRest -i")
    ap.add_argument("-e", "--epsilon", type=float, default=1.0e-4, help="HRest -e")
    ap.add_argument("-v", "--minvar", type=float, default=0.0, help="HRest -v")
    ap.add_argument("-m", "--minseg", type=int, default=3, help="HRest -m")
    ap.add_argument("-w", "--mixfloor", type=float, default=0.0, help="HRest -w (multiples of MINMIX)")
    ap.add_argument("-u", "--update", default="tmvw", help="HRest -u")
    ap.add_argument("-t", "--no-reject", action="store_true", help="HRest -t: keep tokens shorter than the model")
    ap.add_argument("-T", "--trace", type=int, default=1, help="1: the reference's -T 1 lines per model")
    ap.add_argument("--out", help="write every model into this one MMF")
    ap.add_argument("-o", "--outdir", help="write one file per model into this directory (HRest -M)")
    ap.add_argument("--binary", action="store_true", help="HRest -B")
    args = ap.parse_args(argv)
    if not args.out and not args.outdir:
        sys.exit("--out or --outdir is needed")

    mmf = capi.Mmf(files=args.mmf, hmm_list=args.hmmlist, hmm_dir=args.hmmdir)
    mmf.refuse_input_xform("hrest_set")
    if mmf.var_floor is not None:      # SetVFloor would floor with the macro; htkamd_hrest floors every dimension with -v
        sys.exit("hrest_set: the set carries a ~v varFloor1 macro, which htkamd_hrest does not take (it floors with -v alone)")
    pk = mmf.packed()
    files = list(args.data)
    if args.scp:
        files += [phys for _, phys, _, _ in capi.scp_read(args.scp)]
    if not files:
        sys.exit("no data files")
    mlf = capi.Mlf(args.mlf) if args.mlf else None
    want = (args.target_kind or mmf.kind).upper().split("_")
    stat, labels, kind = [], [], 0
    for f in files:
        X, _, kind = capi.parm_read(f)
        base = os.path.splitext(os.path.basename(f))[0]
        labs = mlf.find(base + ".lab") if mlf else capi.labels_read(os.path.join(args.labdir or os.path.dirname(f), base + ".lab"))
        if labs is None:
            sys.exit("no transcription for %s" % f)
        stat.append(X); labels.append(labs)
    need_d, need_a = "D" in want[1:], "A" in want[1:]
    if need_d and not kind & 0o400:
        dX, frame_off, cols = capi.parm_add_qualifiers(stat, hasD=True, hasA=need_a)
    else:
        b = capi._Batch(stat, np.float32)      # the files as they are: one table on the device, and its offsets
        dX, frame_off, cols = b.dev, b.off, b.host.shape[1]
    if cols != pk["vecSize"]:
        sys.exit("data have %d columns, the models %d" % (cols, pk["vecSize"]))
    tokens = tokens_from_labels(pk, mmf.logical, frame_off, labels, seg_reject=False)      # (the call drops the short ones itself)
    names = sorted(mmf.logical, key=lambda n: mmf.logical[n])
    models = sorted({int(mmf.logical[n]) for n in names})
    cfg = capi.hrest_config(args.maxiter, args.epsilon, args.minvar, args.minseg, args.mixfloor * capi.MINMIX, uflags_of(args.update), not args.no_reject)
    model, res = capi.hrest(pk, dX.ptr, int(frame_off[-1]), tokens, models, cfg)
    by_phys = {h: n for n, h in ((n, int(mmf.logical[n])) for n in reversed(names))}
    if args.trace & 1:
        for h, r in zip(models, res):
            print("\n".join(trace_lines(by_phys[h], r)))
    p = model.get_params()
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
    mmf.write(p, one_file=args.out, out_dir=None if args.out else args.outdir, binary=args.binary)
    return model, res


if __name__ == "__main__":
    main()
