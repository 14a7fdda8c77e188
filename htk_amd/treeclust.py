"""HHEd edit scripts restricted to tree-based state clustering: RO, TR, QS, TB and ST (examples/tree_cluster.py, tools/tree_bench.py).

    script = parse_script(open("tree.hed").read())
    run_script(mmf, script, stats_path)           # mmf: capi.Mmf; ties its states, writes script.trees_path if the script has an ST
"""
from __future__ import annotations

import os
import re

from . import capi

COMMANDS = ("RO", "TR", "QS", "TB", "ST")


class Script:
    def __init__(self):
        self.outlier = -1.0          # RO's threshold
        self.stats_path = None       # RO's optional file name
        self.questions = []          # [(name, [pattern, ...])] in QS order
        self.specs = []              # [(threshold, macro root, item list text)] in TB order
        self.trees_path = None       # ST's file name


def _unquote(s: str) -> str:
    s = s.strip()
    if len(s) >= 2 and s[0] in "\"'" and s[-1] == s[0]:
        s = s[1:-1]
    return re.sub(r"\\(.)", r"\1", s)


def _item_list(rest: str, what: str):
    a, b = rest.find("{"), rest.rfind("}")
    if a < 0 or b < a:
        raise capi.HtkAmdError("%s: { item list } expected in '%s'" % (what, rest))
    return rest[:a].strip(), rest[a:b + 1]


def parse_script(text: str) -> Script:
    """One command per line, as HHEd scripts are written.  Any command but RO, TR, QS, TB and ST is refused by name."""
    sc = Script()
    for raw in text.splitlines():
        line = raw.strip()
        if not line:
            continue
        cmd, _, rest = line.partition(" ")
        if len(cmd) != 2 or not cmd.isalpha():
            raise capi.HtkAmdError("edit script: command expected in '%s'" % line)
        cmd = cmd.upper()
        if cmd not in COMMANDS:
            raise capi.HtkAmdError("edit script: command %s is not supported (only %s: tree-based state clustering)" % (cmd, ", ".join(COMMANDS)))
        rest = rest.strip()
        if cmd == "TR":
            continue
        if cmd == "RO":
            f = rest.split(None, 1)
            sc.outlier = float(f[0])
            if len(f) > 1:
                sc.stats_path = _unquote(f[1])
        elif cmd == "ST":
            sc.trees_path = _unquote(rest)
        elif cmd == "QS":
            name, items = _item_list(rest, "QS")
            pats = [_unquote(p) for p in items[1:-1].split(",")]
            sc.questions.append((_unquote(name), pats))
        elif cmd == "TB":
            head, items = _item_list(rest, "TB")
            f = head.split(None, 1)
            if len(f) != 2:
                raise capi.HtkAmdError("TB: threshold and macro name expected in '%s'" % line)
            sc.specs.append((float(f[0]), _unquote(f[1]), items))
    return sc


def run_script(mmf: "capi.Mmf", sc: Script, stats_path=None, merge: bool = True, leaf_stats: bool = True, base_dir: str = ".", stream=None):
    """Apply a parsed script to a loaded set.  stats_path overrides RO's file name; relative file names of the script are taken under base_dir."""
    if not sc.specs:
        raise capi.HtkAmdError("edit script: no TB command")
    sp = stats_path or (os.path.join(base_dir, sc.stats_path) if sc.stats_path else None)
    if sp is None:
        raise capi.HtkAmdError("edit script: no stats loaded (RO names no statistics file and none was given)")
    occ, _ = capi.read_stats(mmf, sp)
    trees = os.path.join(base_dir, sc.trees_path) if sc.trees_path else None
    return mmf.tree_cluster(occ, sc.questions, sc.specs, outlier=sc.outlier, merge=merge, leaf_stats=leaf_stats, trees_path=trees, stream=stream)
