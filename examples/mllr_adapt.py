"""MLLR mean transforms for one speaker through the C ABI -- what
    HERest -C cfg -H mmf -S scp -I mlf -u a -J treedir -K outdir ext -h mask hmmlist
does with HADAPT:TRANSKIND = MLLRMEAN and ADAPTKIND = TREE: one forward-backward pass over the speaker's files, then the transforms over the
regression class tree (HHEd RC's <id>.tree and <id>.base), written as the speaker's transform file.  Example with this repository's fixture:

    python examples/mllr_adapt.py --mmf tests/golden/mllr/hmmdefs --hmmlist tests/golden/mllr/hmmlist --tree tests/golden/mllr/rtree.tree \
        --base tests/golden/mllr/rtree.base --scp tests/golden/mllr/train.scp --datadir tests/golden/mllr --mlf tests/golden/mllr/labels.mlf \
        --blocks 2 4 --split-thresh 245.099 --out /tmp/sp1.mllr

--score-file F prints the sum of F's state scores before and under the transforms (the adapted means serve every scorer, aligner and decoder
until Mllr.restore).  One speaker per call; an alignment under the transforms is what examples/hvite_decode.py does on the adapted model.
"""
import argparse
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from htk_amd import capi  # noqa: E402


def read_tree(tree_path, base_path):
    """capi.RegTree from HHEd RC's two files."""
    kids = {}
    for ln in open(tree_path):
        f = ln.split()
        if f and f[0] == "<NODE>":
            kids[int(f[1])] = (int(f[3]), int(f[4]))
        elif f and f[0] == "<TNODE>":
            kids[int(f[1])] = (0, 0)
    children = [kids[i] for i in range(1, len(kids) + 1)]
    classes = [[(a, int(b), int(c)) for a, b, c in re.findall(r"([^,{}]+)\.state\[(\d+)\]\.mix\[(\d+)\]", m.group(1))]
               for m in re.finditer(r"<CLASS> \d+ \{([^}]*)\}", open(base_path).read())]
    term = [i + 1 for i, k in enumerate(children) if k == (0, 0)]
    return capi.RegTree.from_tables(children, dict(zip(term, classes)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mmf", action="append", required=True); ap.add_argument("--hmmlist", required=True)
    ap.add_argument("--tree", required=True); ap.add_argument("--base", required=True)
    ap.add_argument("--scp", required=True); ap.add_argument("--datadir", default="", help="prefix of the script file's paths")
    ap.add_argument("--mlf", required=True); ap.add_argument("--out", required=True, help="the transform file")
    ap.add_argument("--blocks", nargs="*", type=int, default=None, help="HADAPT:BLOCKSIZE (default: one block)")
    ap.add_argument("--split-thresh", type=float, default=0.0, help="HADAPT:SPLITTHRESH (default 1000)")
    ap.add_argument("--min-occ", type=float, default=0.0, help="HADAPT:MINOCCTHRESH"); ap.add_argument("--no-bias", action="store_true")
    ap.add_argument("--score-file", help="a parameter file to score before and under the transforms")
    args = ap.parse_args(argv)

    mmf = capi.Mmf(files=args.mmf, hmm_list=args.hmmlist)
    tree = read_tree(args.tree, args.base)
    cfg = dict(split_thresh=args.split_thresh, min_occ_thresh=args.min_occ, use_bias=not args.no_bias, blocks=args.blocks)
    capi.Mllr.check(mmf, tree, **cfg)                                   # every refusal, before any data is read
    model = capi.Model(mmf.packed())
    mlf = capi.Mlf(args.mlf)
    files = [l.strip() for l in open(args.scp) if l.strip()]
    feats, seqs = [], []
    for f in files:
        labs = mlf.find(os.path.splitext(f)[0] + ".lab")
        if labs is None:
            sys.exit("no transcription for %s" % f)
        feats.append(capi.parm_read(os.path.join(args.datadir, f))[0])
        seqs.append(np.array([mmf.logical[n] for n, _, _, _ in labs], np.int32))
    batch = capi._Batch(feats, np.float32)
    fb, acc = capi.ForwardBackward(model), capi.Accs(model)
    fb.prepare(batch.dev.ptr.value, batch.off, capi.offsets([len(q) for q in seqs]), np.concatenate(seqs))
    fb.execute(capi.fb_config(), acc)
    for f, st in zip(files, fb.results()[1]):
        if st != 1:
            print("WARNING [-7324]  %s - bad data or over pruning" % f)
    xs = capi.Mllr.estimate(mmf, model, acc, tree, **cfg)
    if xs.status == capi.MLLR_NOSET:
        sys.exit("not enough data to generate transforms: the root's occupation %.3f does not exceed the threshold" % xs.node_occ()[0])
    xs.set_names(os.path.basename(args.out), os.path.basename(args.base))
    xs.write(args.out)
    print("%d transforms at nodes %s; classes -> %s; wrote %s" % (xs.num_xforms, xs.xform_nodes, xs.class_xform, args.out))
    if args.score_file:
        X = capi.parm_read(args.score_file)[0]
        states = np.arange(model.S, dtype=np.int32)
        before = float(model.outp_block(X, states).max(axis=1).sum())
        xs.apply(model)
        print("best state score per frame, summed: %.3f before, %.3f under the transforms" % (before, float(model.outp_block(X, states).max(axis=1).sum())))
        capi.Mllr.restore(model)
    return xs


if __name__ == "__main__":
    main()
