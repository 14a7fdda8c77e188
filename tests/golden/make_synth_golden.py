"""Fixture of tests/test_treesynth_host.py and tests/test_gpu_treesynth.py: what the reference's HHEd (oracle/_ref/HHEd) makes of LT / AU / CO
on the tree-clustering fixture (tests/golden/treeclust: 9 phones a..i, 161 seen triphones).

    python tests/golden/make_synth_golden.py          # needs oracle/_ref/HHEd; rewrites tests/golden/treesynth/

Only data is written: lists, trees files, gzip'd model sets and counts.json.

  full, seen     all 729 triphones x-y+z in a shuffled order; the models hmmdefs defines, in its order
  case A         script 1's RO / QS / TB, then AU full, CO tiedlistA, ST treesA            -> synthA.mmf.gz, tiedlistA, treesA
                 (hmmdefs has one ~t macro per centre phone already -- what "TI T_y {(*-y+*).transP}" would make -- so no TI is needed)
                 the same without CO                                                        -> synthA_au.mmf.gz (the uncompacted set)
                 CO alone on that file as HHEd loads it                                      -> synthA_co.mmf.gz, tiedlistA_co
  case B         the tied set of script 1 (treeclust/tied1.mmf.gz) and treesA in a second run: LT treesA, AU full, CO tiedlistB
                 -> synthB.mmf.gz, tiedlistB (the list must be case A's: LT restores what TB held; the set differs in the last digit of a
                 few gConsts, which the second run computes from variances that went through the text form)
                 LT treesA, ST: the trees file as HHEd writes it back (every question's patterns reversed)  -> treesA.lt_st
  case C         hmmdefs with every transition matrix inline (no ~t macros): script 1, AU full, CO   -> untied.mmf.gz, synthC.mmf.gz,
                 tiedlistC: every synthesised model owns its matrix, so CO merges none of them (EquivHMM compares matrices by identity)
  case D         case B after MU 2 {*.state[2-4].mix} (a run of its own)                    -> mixD.mmf.gz, synthD.mmf.gz, tiedlistD
  case E         a list with `sil`, which has no trees and is not in the set: HHEd's error text        -> counts.json "caseE_error"
                 treesA without the tree b[4] -> treesE2; LT treesE2, AU full: HHEd's error text       -> counts.json "caseE2_error"
"""
from __future__ import annotations

import gzip
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_treeclust_golden as tcg      # noqa: E402

OUT = os.path.join(HERE, "treesynth")
SRC = os.path.join(HERE, "treeclust")
HHED = tcg.HHED


def full_list():
    names = ["%s-%s+%s" % (l, p, r) for p in tcg.PHONES for l in tcg.PHONES for r in tcg.PHONES]
    np.random.RandomState(3).shuffle(names)
    return names


def tb_script(stats="stats") -> str:
    """Script 1 of the tree-clustering fixture without its ST."""
    return "".join(ln + "\n" for ln in tcg.script(1, stats=stats).splitlines() if not ln.startswith("ST ")) + "TR 1\n"


def untie_transitions(text: str) -> str:
    """The model set with every ~t reference replaced by the matrix itself and the ~t macros gone."""
    mats = dict(re.findall(r'~t "([^"]+)"\n(<TRANSP> \d+\n(?: [^\n]*\n)+)', text))
    head, _, rest = text.partition('~h "')
    head = re.sub(r'~t "[^"]+"\n<TRANSP> \d+\n(?: [^\n]*\n)+', "", head)
    rest = re.sub(r'~t "([^"]+)"\n', lambda m: mats[m.group(1)], rest)
    return head + '~h "' + rest


def hhed(work, mmf, lst, script_text, out_mmf, expect_fail=False):
    with open(os.path.join(work, "s.hed"), "w") as f:
        f.write(script_text)
    r = subprocess.run([HHED, "-T", "1", "-H", mmf, "-w", out_mmf, "s.hed", lst], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if expect_fail:
        assert r.returncode != 0, "HHEd was expected to fail:\n" + r.stdout[-2000:]
        return r.stdout
    if r.returncode:
        raise RuntimeError("HHEd failed:\n" + r.stdout[-3000:])
    return r.stdout


def counts(out: str) -> dict:
    d = {}
    m = re.search(r"AU: (\d+) Log/(\d+) Phys created from (\d+) Log/(\d+) Phys", out)
    if m:
        d["AU"] = dict(zip(("log", "phys", "oldLog", "oldPhys"), map(int, m.groups())))
    m = re.search(r"CO: HMMs (\d+) Logical (\d+) Physical", out)
    if m:
        d["CO"] = dict(logical=int(m.group(1)), physical=int(m.group(2)))
    return d


def gz(src, dst):
    with open(src, "rb") as f, open(dst, "wb") as g:
        with gzip.GzipFile(filename="", mode="wb", fileobj=g, mtime=0) as z:
            z.write(f.read())


def main():
    if not os.path.exists(HHED):
        raise SystemExit("oracle/_ref/HHEd is missing: make -C oracle _ref/HHEd where the reference lies")
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    work = tempfile.mkdtemp()
    J = lambda n: os.path.join(work, n)      # noqa: E731
    text = gzip.open(os.path.join(SRC, "hmmdefs.gz"), "rt").read()
    seen = re.findall(r'^~h "([^"]+)"', text, flags=re.M)
    full = full_list()
    assert set(seen) <= set(full) and len(full) == 729
    for n, data in (("hmmdefs", text), ("seen", "\n".join(seen) + "\n"), ("full", "\n".join(full) + "\n"), ("untied.mmf", untie_transitions(text)),
                    ("tied1.mmf", gzip.open(os.path.join(SRC, "tied1.mmf.gz"), "rt").read()), ("fullE", "\n".join(full[:40] + ["sil"] + full[40:]) + "\n")):
        with open(J(n), "w") as f:
            f.write(data)
    shutil.copy(os.path.join(SRC, "stats"), J("stats"))
    info = {}
    # case A
    info["caseA"] = counts(hhed(work, "hmmdefs", "seen", tb_script() + "AU full\nCO tiedlistA\nST treesA\n", "synthA.mmf"))
    assert open(J("treesA")).read() == open(os.path.join(SRC, "trees1")).read(), "ST after AU shows other trees than ST after TB"
    hhed(work, "hmmdefs", "seen", tb_script() + "AU full\n", "synthA_au.mmf")
    info["caseA_co"] = counts(hhed(work, "synthA_au.mmf", "full", "CO tiedlistA_co\n", "synthA_co.mmf"))
    info["caseA_co"]["list_equals_caseA"] = open(J("tiedlistA_co")).read() == open(J("tiedlistA")).read()
    # case B
    info["caseB"] = counts(hhed(work, "tied1.mmf", "seen", "LT treesA\nAU full\nCO tiedlistB\n", "synthB.mmf"))
    assert open(J("tiedlistB")).read() == open(J("tiedlistA")).read(), "LT does not restore what TB held"
    info["caseB"]["set_equals_caseA"] = open(J("synthB.mmf")).read() == open(J("synthA.mmf")).read()
    hhed(work, "tied1.mmf", "seen", "LT treesA\nST treesA.lt_st\n", "unused.mmf")
    # case C
    info["caseC"] = counts(hhed(work, "untied.mmf", "seen", tb_script() + "AU full\nCO tiedlistC\n", "synthC.mmf"))
    assert info["caseC"]["CO"]["physical"] > info["caseA"]["CO"]["physical"], "untied matrices change nothing: case C tests nothing"
    # case D
    hhed(work, "tied1.mmf", "seen", "MU 2 {*.state[2-4].mix}\n", "mixD.mmf")
    info["caseD"] = counts(hhed(work, "mixD.mmf", "seen", "LT treesA\nAU full\nCO tiedlistD\n", "synthD.mmf"))
    # case E
    out = hhed(work, "tied1.mmf", "seen", "LT treesA\nAU fullE\n", "unused.mmf", expect_fail=True)
    err = [ln.strip() for ln in out.splitlines() if "ERROR" in ln]
    info["caseE_error"] = err[0] if err else out.strip().splitlines()[-1]
    assert "sil" in info["caseE_error"]
    trees = open(J("treesA")).read()
    cut = re.sub(r"(?ms)^b\[4\]\n\{.*?^\}\n\n", "", trees)
    assert cut != trees
    with open(J("treesE2"), "w") as f:
        f.write(cut)
    out = hhed(work, "tied1.mmf", "seen", "LT treesE2\nAU full\n", "unused.mmf", expect_fail=True)
    info["caseE2_error"] = [ln.strip() for ln in out.splitlines() if "ERROR" in ln][0]
    assert "state 4" in info["caseE2_error"]
    for n in ("seen", "full", "fullE", "treesE2", "tiedlistA", "tiedlistA_co", "tiedlistB", "tiedlistC", "tiedlistD", "treesA", "treesA.lt_st"):
        shutil.copy(J(n), os.path.join(OUT, n))
    for n in ("synthA.mmf", "synthA_au.mmf", "synthA_co.mmf", "synthB.mmf", "untied.mmf", "synthC.mmf", "mixD.mmf", "synthD.mmf"):
        gz(J(n), os.path.join(OUT, n + ".gz"))
    with open(os.path.join(OUT, "counts.json"), "w") as f:
        json.dump(info, f, indent=1, sort_keys=True)
        f.write("\n")
    shutil.rmtree(work)
    print("treesynth golden:", json.dumps(info), {n: os.path.getsize(os.path.join(OUT, n)) for n in sorted(os.listdir(OUT))})


if __name__ == "__main__":
    main()
