"""HHEd edit scripts restricted to state clustering and tying: RO, LS, TR, QS, TB, ST (tree-based) and TC, NC, TI (data-driven), and -- for
a caller that asks for them, parse_script(text, synth=True) -- LT, AU, CO: the unseen triphones from the trees and the compacted set
(examples/tree_cluster.py, tools/tree_bench.py, tools/synth_bench.py).  parse_script(text, regtree=True) takes RC as well: the regression
class tree and its base classes (tools/regtree_bench.py).

    script = parse_script(open("tree.hed").read())
    run_script(mmf, script, stats_path)           # mmf: capi.Mmf; ties its states, writes script.trees_path if the script has an ST
"""
from __future__ import annotations

import os
import re

from . import capi

COMMANDS = ("RO", "TR", "QS", "TB", "ST", "TC", "NC", "TI", "LS")
TREE_ONLY = ("RO", "TR", "QS", "TB", "ST")
SYNTH = ("LT", "AU", "CO")
_RC_ARGS = re.compile(r"""\s*([+-]?\d+)\s+("(?:\\.|[^"\\])*"|'(?:\\.|[^'\\])*'|\S+)(.*)$""")


class Script:
    def __init__(self):
        self.outlier = -1.0          # RO's threshold
        self.stats_path = None       # RO's optional file name
        self.questions = []          # [(name, [pattern, ...])] in QS order
        self.specs = []              # [(threshold, macro root, item list text)] in TB order
        self.trees_path = None       # ST's file name
        self.commands = []           # every command in script order: ("RO", threshold, file | None), ("LS", file), ("QS", name, patterns),
                                     # ("TB", threshold, macro, items), ("TC" | "NC", value, macro, items), ("TI", macro, items), ("ST", file),
                                     # and with synth=True ("LT", file), ("AU", file), ("CO", file); with regtree=True
                                     # ("RC", terminals, identifier, item list | None)


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


def parse_script(text: str, synth: bool = False, regtree: bool = False) -> Script:
    """One command per line, as HHEd scripts are written; the commands are kept in script order (Script.commands).  Any command but
    RO, LS, TR, QS, TB, ST, TC, NC and TI is refused by name -- and with synth=True LT, AU and CO are taken, too, with regtree=True
    `RC N identifier [itemlist]`."""
    sc = Script()
    for raw in text.splitlines():
        line = raw.strip()
        if not line:
            continue
        cmd, _, rest = line.partition(" ")
        if len(cmd) != 2 or not cmd.isalpha():
            raise capi.HtkAmdError("edit script: command expected in '%s'" % line)
        cmd = cmd.upper()
        if synth and cmd in SYNTH:
            if not rest.strip():
                raise capi.HtkAmdError("%s: file name expected" % cmd)
            sc.commands.append((cmd, _unquote(rest)))
            continue
        if regtree and cmd == "RC":
            m = _RC_ARGS.match(rest)      # the identifier as HHEd's ChkedAlpha reads a string: quoted (white space allowed inside) or up to white space
            if not m:
                raise capi.HtkAmdError("RC: number of terminal nodes and identifier expected in '%s'" % line)
            n, ident, items = m.group(1), m.group(2), m.group(3).strip()
            if not 0 <= int(n) <= 256:
                raise capi.HtkAmdError("RC: maximum number of terminal nodes is 256, got %s" % n)
            if items and not items.startswith("{"):
                raise capi.HtkAmdError("RC: { item list } expected in '%s'" % items)
            sc.commands.append(("RC", int(n), _unquote(ident), items or None))
            continue
        if cmd not in COMMANDS:
            raise capi.HtkAmdError("edit script: command %s is not supported (only %s: state clustering and tying)" % (cmd, ", ".join(COMMANDS)))
        rest = rest.strip()
        if cmd == "TR":
            continue
        if cmd == "RO":
            f = rest.split(None, 1)
            sc.outlier = float(f[0])
            if len(f) > 1:
                sc.stats_path = _unquote(f[1])
            sc.commands.append(("RO", sc.outlier, _unquote(f[1]) if len(f) > 1 else None))
        elif cmd == "LS":
            if not rest:
                raise capi.HtkAmdError("LS: statistics file name expected")
            sc.commands.append(("LS", _unquote(rest)))
        elif cmd == "ST":
            sc.trees_path = _unquote(rest)
            sc.commands.append(("ST", sc.trees_path))
        elif cmd == "QS":
            name, items = _item_list(rest, "QS")
            pats = [_unquote(p) for p in items[1:-1].split(",")]
            sc.questions.append((_unquote(name), pats))
            sc.commands.append(("QS",) + sc.questions[-1])
        elif cmd == "TB":
            head, items = _item_list(rest, "TB")
            f = head.split(None, 1)
            if len(f) != 2:
                raise capi.HtkAmdError("TB: threshold and macro name expected in '%s'" % line)
            sc.specs.append((float(f[0]), _unquote(f[1]), items))
            sc.commands.append(("TB",) + sc.specs[-1])
        elif cmd in ("TC", "NC"):
            head, items = _item_list(rest, cmd)
            f = head.split(None, 1)
            if len(f) != 2:
                raise capi.HtkAmdError("%s: %s and macro name expected in '%s'" % (cmd, "threshold" if cmd == "TC" else "number of clusters", line))
            sc.commands.append((cmd, float(f[0]) if cmd == "TC" else int(f[0]), _unquote(f[1]), items))
        elif cmd == "TI":
            head, items = _item_list(rest, "TI")
            if not head:
                raise capi.HtkAmdError("TI: macro name expected in '%s'" % line)
            sc.commands.append(("TI", _unquote(head), items))
    return sc


def run_script(mmf: "capi.Mmf", sc: Script, stats_path=None, merge: bool = True, leaf_stats: bool = True, base_dir: str = ".", stream=None):
    """Apply a parsed script to a loaded set.  stats_path overrides RO's file name; relative file names of the script are taken under base_dir.
    A script of RO TR QS TB ST alone is one tree_cluster call.  Otherwise the commands run in script order, consecutive TC / NC commands
    as one device call and consecutive TB commands as another; returns the list of what the calls returned.  In a script with LT, AU or
    CO (parse_script(.., synth=True)) the trees stay on the set as in HHEd: AU after TB or LT uses them, ST writes all of them where it
    stands; AU returns (seen, unseen), CO (logical, physical).  RC (parse_script(.., regtree=True)) writes identifier.tree and
    identifier.base under base_dir from the statistics loaded at that point and returns the capi.RegTree."""
    if all(c[0] in TREE_ONLY for c in sc.commands):
        if not sc.specs:
            raise capi.HtkAmdError("edit script: no TB command")
        sp = stats_path or (os.path.join(base_dir, sc.stats_path) if sc.stats_path else None)
        if sp is None:
            raise capi.HtkAmdError("edit script: no stats loaded (RO names no statistics file and none was given)")
        occ, _ = capi.read_stats(mmf, sp)
        trees = os.path.join(base_dir, sc.trees_path) if sc.trees_path else None
        return mmf.tree_cluster(occ, sc.questions, sc.specs, outlier=sc.outlier, merge=merge, leaf_stats=leaf_stats, trees_path=trees, stream=stream)
    cmds = sc.commands
    tb_groups = sum(1 for k, c in enumerate(cmds) if c[0] == "TB" and (k == 0 or cmds[k - 1][0] != "TB"))
    synth = any(c[0] in SYNTH for c in cmds)
    if tb_groups > 1 and sc.trees_path and not synth:
        raise capi.HtkAmdError("edit script: ST after TB commands that other commands separate is not supported (the trees of one run of TB commands are written)")
    loaded, outlier, questions, out = None, -1.0, [], []

    def occupations():
        # the set's states are renumbered by every tying call: the occupations are read again for the numbering of the moment
        return capi.read_stats(mmf, loaded)[0] if loaded else None

    k = 0
    while k < len(cmds):
        c = cmds[k]
        if c[0] == "RO":
            outlier = c[1]
            name = stats_path or (os.path.join(base_dir, c[2]) if c[2] else None)
            if name:
                loaded = name
        elif c[0] == "LS":
            loaded = stats_path or os.path.join(base_dir, c[1])
        elif c[0] == "QS":
            questions.append((c[1], c[2]))
        elif c[0] in ("TC", "NC", "TB"):
            kinds = ("TB",) if c[0] == "TB" else ("TC", "NC")
            e = k
            while e < len(cmds) and cmds[e][0] in kinds:
                e += 1
            if c[0] == "TB":
                if not loaded:
                    raise capi.HtkAmdError("edit script: no stats loaded (no RO or LS command names a statistics file before TB and none was given)")
                trees = os.path.join(base_dir, sc.trees_path) if sc.trees_path and not synth else None
                out.append(mmf.tree_cluster(occupations(), list(questions), [x[1:] for x in cmds[k:e]], outlier=outlier, merge=merge, leaf_stats=leaf_stats,
                                            trees_path=trees, stream=stream))
            else:
                out.append(mmf.data_cluster(occupations(), cmds[k:e], outlier=outlier, stream=stream))
            k = e
            continue
        elif c[0] == "TI":
            out.append(mmf.tie(c[1], c[2]))
        elif c[0] == "RC":
            if not loaded:
                raise capi.HtkAmdError("edit script: no stats loaded (no RO or LS command names a statistics file before RC and none was given)")
            tree = mmf.regtree(occupations(), c[1], c[3], stream=stream)
            tree.write(c[2], base_dir)
            out.append(tree)
        elif c[0] == "LT":
            mmf.load_trees(os.path.join(base_dir, c[1]))
        elif c[0] == "AU":
            out.append(mmf.add_unseen(os.path.join(base_dir, c[1]), stream=stream))
        elif c[0] == "CO":
            out.append(mmf.compact(os.path.join(base_dir, c[1])))
        elif c[0] == "ST" and synth:
            mmf.save_trees(os.path.join(base_dir, c[1]))
        k += 1
    return out
