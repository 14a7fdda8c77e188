"""The cases of the regression class tree tests (tests/test_regtree_host.py, tests/test_gpu_regtree.py) and of their fixture generator
(tests/golden/make_regtree_golden.py): which sets (htk_amd/regtree_sets.py writes them), which RC scripts, and how HHEd and the library are
run over them."""
import os
import re
import subprocess

from htk_amd.regtree_sets import IDENT, names_for, write_script, write_set      # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "regtree")
HHED = os.path.join(ROOT, "oracle", "_ref", "HHEd")

# the committed cases: name -> (write_set arguments, number of terminals, item list)
CASES = {
    # a: D = 5 (no lane multiple), 3 models x 3 states x 2 mixtures, N = 4
    "a":    (dict(names=names_for(3), n_emit=3, n_mix=2, D=5, seed=1), 4, None),
    # b: 70 and 130 Gaussians in the root (over one and over two wavefronts), N = 8
    "b70":  (dict(names=names_for(7), n_emit=5, n_mix=2, D=3, seed=2), 8, None),
    "b130": (dict(names=names_for(13), n_emit=5, n_mix=2, D=3, seed=12), 8, None),
    # c: a sil model's states go to the non-speech child
    "c":    (dict(names=names_for(6, sil=True), n_emit=3, n_mix=2, D=3, seed=3), 4, "{sil.state[2-4].mix}"),
    # d: more terminals asked for than splits are possible
    "d":    (dict(names=names_for(5), n_emit=4, n_mix=2, D=4, seed=4), 32, None),
    # e: Gaussians with identical means, and an exact tie between the two seeds (see write_set's dyadic)
    "e":    (dict(names=names_for(6), n_emit=3, n_mix=2, D=3, seed=5, dyadic=True, twins=(((2, 1, 0), (4, 2, 0)),)), 4, None),
    # f: a state with zero occupation in the statistics
    "f":    (dict(names=names_for(5), n_emit=3, n_mix=2, D=3, seed=6, occ_zero=((1, 1), (3, 0))), 4, None),
    # g: a ~s-tied state and a ~m-shared Gaussian, each reached from two models
    "g":    (dict(names=names_for(6), n_emit=3, n_mix=2, D=3, seed=7, tied=True), 4, None),
    # h: a split that needs more than 10 iterations
    "h":    (dict(names=names_for(40), n_emit=3, n_mix=4, D=4, seed=8, clusters=5), 2, None),
}

# Further scripts over a case's set that split nothing, so no device is needed: (case, identifier) -> (number of terminals, item list).
# The script is <identifier>.hed, HHEd's files <identifier>.tree and <identifier>.base beside the case's own.
#   unsplit: the lists of InitRegTree's scan as they stand (RC 1; RC 2 behind the case's non-speech list)
#   items:   an item list in every form PItemList takes for pdfs: a parenthesised model list, quoted names, ? * and % patterns (a % makes
#            a name a pattern, but DoMatch takes it literally: 'm%5' names no model), an index list [2,4] beside ranges, several items
NO_SPLIT = {
    ("a", "unsplit"): (1, None),
    ("c", "unsplit"): (2, "{sil.state[2-4].mix}"),
    ("c", "items"):   (2, '{ ("sil","m0?").state[2,4].mix, m03.state[3].mix,\'m%5\'.state[2-3].mix , "m*5".state[3-3].mix}'),
}
# what ("c", "items") names, written out one state at a time
ITEMS_PLAIN = "{" + ",".join("%s.state[%d].mix" % (m, j) for m, js in (("sil", (2, 4)), ("m01", (2, 4)), ("m02", (2, 4)), ("m03", (2, 3, 4)), ("m04", (2, 4)),
                                                                       ("m05", (2, 3, 4))) for j in js) + "}"


def make_case(d, name):
    args, n, items = CASES[name]
    write_set(d, **args)
    write_script(d, n, items)
    for (case, ident), (n2, items2) in NO_SPLIT.items():
        if case == name:
            write_script(d, n2, items2, ident=ident, name=ident + ".hed")
    return n, items


def run_hhed(d, trace=0, script="rc.hed"):
    """The reference's HHEd over the case in `d`: the script's .tree and .base files land there; returns its output."""
    r = subprocess.run([HHED, "-T", str(trace), "-H", "hmmdefs", "-M", ".", script, "hmmlist"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        raise RuntimeError("HHEd failed (%d):\n%s" % (r.returncode, r.stdout[-3000:]))
    return r.stdout


def parse_tree(text):
    """children [(left, right)] by node from 1 of a .tree file."""
    kids = {}
    for ln in text.splitlines():
        f = ln.split()
        if f and f[0] == "<NODE>":
            kids[int(f[1])] = (int(f[3]), int(f[4]))
        elif f and f[0] == "<TNODE>":
            kids[int(f[1])] = (0, 0)
    return [kids[i] for i in range(1, len(kids) + 1)]


def parse_base(text):
    """[[(model, state, mix), ...] per class] of a .base file."""
    out = []
    for m in re.finditer(r"<CLASS> \d+ \{([^}]*)\}", text):
        out.append([(a, int(b), int(c)) for a, b, c in re.findall(r"([^,{}]+)\.state\[(\d+)\]\.mix\[(\d+)\]", m.group(1))])
    return out


def run_library(d, out_dir, stream=None, script="rc.hed"):
    """The case in `d` through the edit-script runner; the two files land in out_dir.  Returns the capi.RegTree."""
    from htk_amd import capi, treeclust
    sc = treeclust.parse_script(open(os.path.join(d, script)).read(), regtree=True)
    mmf = capi.Mmf([os.path.join(d, "hmmdefs")], hmm_list=os.path.join(d, "hmmlist"))
    return treeclust.run_script(mmf, sc, stats_path=os.path.join(d, "stats"), base_dir=str(out_dir), stream=stream)[-1]
