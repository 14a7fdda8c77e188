"""Tree-based state tying (HHEd's RO / QS / TB / ST) on the device: the step between cloned single-Gaussian triphones plus an HERest -s
statistics file and a tied-state set ready for mix-up.

    python examples/tree_cluster.py tree.hed hmmdefs triphones stats -o tied.mmf [--trees trees] [--no-merge] [--no-leaf-stats]

The edit script may hold RO, LS, TR, QS, TB and ST, and for data-driven clustering TC, NC and TI (furthest-neighbour clustering of the
listed states on the device; a script needs no TB then); any other command is refused by name.  --no-merge / --no-leaf-stats are HHEd's
configuration variables TREEMERGE = F / USELEAFSTATS = F.  LT, AU and CO are taken, too: "... TB ... AU fulllist CO tiedlist ST trees"
synthesises the unseen triphones of fulllist from the trees on the device and compacts the set; in a second run "LT trees AU fulllist
CO tiedlist" does the same from a saved trees file (MU inside a script stays refused)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htk_amd import capi, treeclust


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("script"); ap.add_argument("mmf"); ap.add_argument("hmmlist"); ap.add_argument("stats")
    ap.add_argument("-o", "--out", required=True, help="the tied model set (one master file)")
    ap.add_argument("--trees", help="trees file (overrides the script's ST)")
    ap.add_argument("--no-merge", action="store_true"); ap.add_argument("--no-leaf-stats", action="store_true")
    a = ap.parse_args(argv)
    sc = treeclust.parse_script(open(a.script).read(), synth=True, regtree=True)
    if a.trees:
        sc.trees_path = os.path.abspath(a.trees)
    mmf = capi.Mmf([a.mmf], hmm_list=a.hmmlist)
    before = mmf.desc.numStates
    warn = treeclust.run_script(mmf, sc, stats_path=a.stats, merge=not a.no_merge, leaf_stats=not a.no_leaf_stats, base_dir=os.path.dirname(os.path.abspath(a.script)))
    if isinstance(warn, str):
        print(warn, file=sys.stderr)
    mmf.write(mmf.packed(), one_file=a.out)
    for c, r in zip([c for c in sc.commands if c[0] in ("AU", "CO")], [r for r in (warn if isinstance(warn, list) else []) if isinstance(r, tuple)]):
        print("tree_cluster: %s %s: %s" % (c[0], c[1], "%d seen, %d unseen" % r if c[0] == "AU" else "%d logical, %d physical" % r))
    print("tree_cluster: %d trees, %d TC / NC commands, %d states -> %d" % (len(sc.specs), sum(c[0] in ("TC", "NC") for c in sc.commands), before, mmf.desc.numStates))


if __name__ == "__main__":
    main()
