"""The synthesis fixture (tests/golden/treesynth, made by tests/golden/make_synth_golden.py from HHEd's LT / AU / CO) as files."""
import gzip
import json
import os

import treeclust_util as tu

ROOT = tu.ROOT
GS = os.path.join(ROOT, "tests", "golden", "treesynth")
COUNTS = json.load(open(os.path.join(GS, "counts.json")))
LISTS = ("seen", "full", "fullE", "treesA", "treesE2")


def golden_bytes(name: str) -> bytes:
    p = os.path.join(GS, name)
    if os.path.exists(p):
        return open(p, "rb").read()
    return gzip.open(p + ".gz", "rb").read()


def workdir(tmp, mmf_name: str) -> str:
    """A directory with the model set `mmf_name` (of this fixture, or hmmdefs / tied1.mmf of the tree-clustering one) as in.mmf, the lists,
    the trees files and the statistics file; returns its path."""
    w = str(tmp)
    with open(os.path.join(w, "in.mmf"), "wb") as f:
        f.write(tu.golden_bytes(mmf_name) if mmf_name in ("hmmdefs", "tied1.mmf") else golden_bytes(mmf_name))
    for n in LISTS:
        with open(os.path.join(w, n), "wb") as f:
            f.write(golden_bytes(n))
    with open(os.path.join(w, "stats"), "wb") as f:
        f.write(tu.golden_bytes("stats"))
    return w


def tb_script() -> str:
    """Script 1 of the tree-clustering fixture without its ST (the RO / QS / TB part of cases A and C)."""
    return "".join(ln + "\n" for ln in tu.golden_bytes("script1.hed").decode().splitlines() if not ln.startswith("ST "))


def first_difference(mine: bytes, ref: bytes) -> str:
    """Where two model sets part: the model (or macro) and the line."""
    a, b = mine.decode(errors="replace").splitlines(), ref.decode(errors="replace").splitlines()
    where = "(before any macro)"
    for k in range(min(len(a), len(b))):
        if b[k].startswith("~"):
            where = b[k]
        if a[k] != b[k]:
            return "line %d, in %s: mine %r, reference %r" % (k + 1, where, a[k], b[k])
    return "lengths differ: mine %d lines, reference %d" % (len(a), len(b))


def same(mine: bytes, ref: bytes, what: str):
    assert mine == ref, "%s: %s" % (what, first_difference(mine, ref))
