#!/usr/bin/env python3
"""HInit for EVERY model of a list in one call (htkamd_hinit) -- the data flow of, for each model X of the list,
    HInit -C cfg -S scp -L labdir|-I mlf -l X -o X -i n -e f -v f -m n -u tmvw [-n] -M outdir protodir/X
with every model's tokens taken from its own labels (one label per model; -l with a label shared by several models is not served).
All models go into one library call: uniform segmentation, FlatCluster, alignment, best components, statistics and updates run on the
device for all of them side by side.  Example with the HTKDemo fixtures of this repository:

    python examples/hinit_set.py --hmmlist tests/golden/demo/bcplist --hmmdir tests/golden/demo/proto \
        --data tests/golden/demo/train/*.mfc --labdir tests/golden/demo/labels --target-kind MFCC_E_D --maxiter 10 --outdir /tmp/hmm0

    from examples.hinit_set import tokens_from_labels          # rows of (first frame, frames, physical model) in the reference's order
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from htk_amd import capi  # noqa: E402

STATUS_TEXT = {capi.HINIT_EFEWSEGS: "too few training tokens (-m)", capi.HINIT_ESHORT: "a token shorter than the model",
               capi.HINIT_ENOMIX: "FindBestMixes: no best mix", capi.HINIT_ENOPATH: "no path found in a token",
               capi.HINIT_EZEROOCC: "a component or state without data", capi.HINIT_ECLUSTER: "FlatCluster could not make the clusters"}


def tokens_from_labels(pk, logical, frame_off, labels, frame_dur=100000, seg_reject=True):
    """The tokens of every model: per file (file order) its label segments (label order) whose name is a model of the list, by the
    rule of examples/hrest_model.py::segments_of -- frames start // frame_dur .. min(end // frame_dur, last frame), kept when the
    segment is not empty and (seg_reject) has at least as many frames as the model has emitting states.  frame_off[i]: first row of
    file i in the table ([files + 1]).  Returns int32 [n, 3]: first row, frames, physical model."""
    rows = []
    for i, labs in enumerate(labels):
        T = int(frame_off[i + 1] - frame_off[i])
        for lab, start, end, _ in labs:
            if lab not in logical:
                continue
            h = int(logical[lab])
            n_emit = int(pk["hmmStateOff"][h + 1] - pk["hmmStateOff"][h])
            st, en = int(start // frame_dur), min(int(end // frame_dur), T - 1)
            if st <= en and (en - st + 1 >= n_emit or not seg_reject):
                rows.append((int(frame_off[i]) + st, en - st + 1, h))
    return np.array(rows, np.int32).reshape(-1, 3)


def uflags_of(text):
    bits = dict(m=capi.UPMEANS, v=capi.UPVARS, t=capi.UPTRANS, w=capi.UPMIXES)
    try:
        return sum({bits[c] for c in text})
    except KeyError as e:
        sys.exit("-u takes the letters t m v w, not %s" % e)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hmmlist", required=True)
    ap.add_argument("--mmf", action="append", default=[], help="master macro file(s) with the prototypes")
    ap.add_argument("--hmmdir", help="directory with one prototype per model")
    ap.add_argument("--scp", help="script file: one parameter file per line (HInit -S)")
    ap.add_argument("--data", nargs="*", default=[], help="parameter files")
    ap.add_argument("--labdir", help="directory of label files (HInit -L)")
    ap.add_argument("--mlf", help="master label file (HInit -I)")
    ap.add_argument("--target-kind", default=None, help="e.g. MFCC_E_D: qualifiers _D/_A missing in the files are computed (TARGETKIND)")
    ap.add_argument("--maxiter", type=int, default=20, help="HInit -i")
    ap.add_argument("--epsilon", type=float, default=1.0e-4, help="HInit -e")
    ap.add_argument("--minvar", type=float, default=1.0e-2, help="HInit -v")
    ap.add_argument("--minseg", type=int, default=3, help="HInit -m")
    ap.add_argument("--mixfloor", type=float, default=0.0, help="HInit -w (multiples of MINMIX)")
    ap.add_argument("--update", default="tmvw", help="HInit -u")
    ap.add_argument("--no-uniform", action="store_true", help="HInit -n: update the models as they are, no uniform segmentation")
    ap.add_argument("--out", help="write every model into this one MMF")
    ap.add_argument("--outdir", help="write one file per model into this directory (HInit -M)")
    ap.add_argument("--binary", action="store_true", help="HInit -B")
    args = ap.parse_args(argv)
    if not args.out and not args.outdir:
        sys.exit("--out or --outdir is needed")

    mmf = capi.Mmf(files=args.mmf, hmm_list=args.hmmlist, hmm_dir=args.hmmdir)
    mmf.refuse_input_xform("hinit_set")
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
    tokens = tokens_from_labels(pk, mmf.logical, frame_off, labels)
    names = sorted(mmf.logical, key=lambda n: mmf.logical[n])
    models = sorted({int(mmf.logical[n]) for n in names})
    cfg = capi.hinit_config(args.maxiter, args.epsilon, args.minvar, args.minseg, args.mixfloor * capi.MINMIX, uflags_of(args.update), not args.no_uniform)
    model, res = capi.hinit(pk, dX.ptr, int(frame_off[-1]), tokens, models, cfg)
    by_phys = {h: n for n, h in ((n, int(mmf.logical[n])) for n in reversed(names))}
    for h, r in zip(models, res):
        for k, p in enumerate(r["logP"]):
            print("HInit %s: Iteration %d: Average LogP =%12.5f" % (by_phys[h], k + 1, p))
        if r["status"] != capi.HINIT_OK:
            print("HInit %s: ERROR [+%d] %s: the model is written as it came" % (by_phys[h], r["status"], STATUS_TEXT.get(r["status"], "")))
        else:
            print("HInit %s: Estimation %s at iteration %d" % (by_phys[h], "converged" if r["converged"] else "aborted", r["passes"] + 1))      # (the reference prints its loop counter, one past the last pass)
    p = model.get_params()
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
    mmf.write(p, one_file=args.out, out_dir=None if args.out else args.outdir, binary=args.binary)
    return model, res


if __name__ == "__main__":
    main()
