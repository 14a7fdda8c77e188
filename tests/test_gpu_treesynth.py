"""Unseen triphones from the trees on the device (htk_amd/csrc/treesynth.hip + htk_amd/host/treesynth.c) against the reference's HHEd:
the wildcard matching byte for byte against DoMatch restated, the walks against a walk of the same tables in Python, and HHEd's LT / AU /
CO outputs byte for byte -- the committed ones (tests/golden/make_synth_golden.py) and HHEd run on the spot where its binary is there."""
import importlib.util
import os
import re

import numpy as np
import pytest

import treeclust_util as tu
import treesynth_util as su
from treeclust_util import ROOT

pytestmark = pytest.mark.gpu

HHED = os.path.join(ROOT, "oracle", "_ref", "HHEd")
MAXNAME = 99


def do_match(s: str, p: str) -> bool:
    """DoMatch / RMatch (HShell.c:1787-1816) as the reference writes it: recursive, '*' any run (also empty), '?' one character."""
    if not p:
        return not s
    if p[0] == "*":
        return do_match(s, p[1:]) or (bool(s) and do_match(s[1:], p))
    return bool(s) and (p[0] == "?" or p[0] == s[0]) and do_match(s[1:], p[1:])


def answers(names, questions):
    return np.array([[any(do_match(n, p) for p in pats) for n in names] for _, pats in questions], np.uint8)


QUESTIONS = [("any", ["*"]), ("left_a", ["a-*"]), ("right_a", ["*+a"]), ("centre_a", ["*-a+*"]), ("one_left", ["?-a+*"]),
             ("longer", ["a-b+c-d+e-f"]), ("plain", ["a-b+c"]), ("backtrack", ["*a*b*"]), ("trailing", ["a-b+c*"]), ("stars", ["**"]),
             ("q_end", ["a-b+?"]), ("q_only", ["?"]), ("qq", ["??"]), ("star_q", ["*?"]), ("mid", ["a*c"]), ("two", ["x*", "*b"]),
             ("many", ["z%d-*" % k for k in range(64)] + ["*+i"]), ("none", ["q-q+q"]), ("tail_star", ["*-*+*", "nothing"]), ("long_pat", ["*" + "y" * 97 + "?"])]
SPECIAL = ["xaxab", "a", "b", "ab", "a-b+c", "a-b+", "a-b+cd", "xab", "xaxa", "aab", "axb", "a-a+a", "x" + "y" * (MAXNAME - 1), "y" * MAXNAME, "c", "a+c", "abc"]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 729])
def test_name_answers_are_do_match_s(native, N):
    full = su.golden_bytes("full").decode().split()
    names = (SPECIAL + full)[:N] if N > 1 else ["xaxab"]
    if N >= 65:
        names[N - 1], names[64] = SPECIAL[0], SPECIAL[12]                          # the last lane in use, the first of the second wavefront
    assert len(names) == N and max(len(n) for n in names) <= MAXNAME
    want = answers(names, QUESTIONS)
    got = native.name_question_answers(names, QUESTIONS)
    assert got.shape == want.shape and np.array_equal(got, want), [(QUESTIONS[q][0], names[n]) for q, n in np.argwhere(got != want)[:8]]
    if N == 729:
        assert want[7, names.index("xaxab")] == 1 and want[7, names.index("xaxa")] == 0 and want[5].sum() == 0 and want[16].sum() > 0
        one = native.name_question_answers(names, QUESTIONS[16:17])              # a question block of its own, 65 patterns
        assert np.array_equal(one, want[16:17])


def test_name_answers_refusals(native):
    with pytest.raises(native.HtkAmdError, match=r"has 100 characters \(at most 99"):
        native.name_question_answers(["a-b+c", "z" * (MAXNAME + 1)], QUESTIONS[:2])
    with pytest.raises(native.HtkAmdError, match="question 1 has no name or no pattern"):
        native.name_question_answers(["a-b+c"], [("q", ["*"]), ("r", [])])
    with pytest.raises(native.HtkAmdError, match="name 1 is empty"):
        native.name_question_answers(["a-b+c", ""], QUESTIONS[:2])


def parse_trees(text: str):
    """({question: patterns}, {(base, state): (nodes {number: (question, no, yes)}, single leaf or None)}) of an ST file."""
    qs, trees = {}, {}
    for m in re.finditer(r"(?m)^QS '([^']+)' \{ (.*) \}$", text):
        qs[m.group(1)] = [p.strip('"') for p in m.group(2).split(",")]
    for m in re.finditer(r"(?m)^(\w+)\[(\d+)\]\n(?:\{\n(.*?)^\}|\s+\"([^\"]+)\")", text, flags=re.S):
        nodes = {}
        for ln in (m.group(3) or "").splitlines():
            f = ln.split()
            nodes[-int(f[0])] = (f[1].strip("'"), f[2].strip('"'), f[3].strip('"'))
        trees[(m.group(1), int(m.group(2)))] = (nodes, m.group(4))
    return qs, trees


def walk(qs, tree, name):
    nodes, single = tree
    if single:
        return single
    cur = 0
    while True:
        q, no, yes = nodes[cur]
        nxt = yes if any(do_match(name, p) for p in qs[q]) else no
        if not re.fullmatch(r"-\d+", nxt):
            return nxt
        cur = -int(nxt)


EXTRA_TREES = "zz[2]\n   \"ST_a_2_1\"\n\nzz[3]\n{\n   0   'L_Vowel'   \"ST_a_3_1\"   \"ST_b_3_1\" \n}\n\n"


@pytest.fixture(scope="module")
def tied_set(native, tmp_path_factory):
    w = su.workdir(tmp_path_factory.mktemp("synth"), "tied1.mmf")
    m = native.Mmf([os.path.join(w, "in.mmf")], hmm_list=os.path.join(w, "seen"))
    m.load_trees(os.path.join(w, "treesA"))
    with open(os.path.join(w, "extra"), "w") as f:
        f.write(EXTRA_TREES)
    m.load_trees(os.path.join(w, "extra"))                                       # no questions of its own: the held ones serve
    return m, w


def test_tree_descend_is_a_walk_of_the_tables(native, tied_set):
    m, w = tied_set
    text = su.golden_bytes("treesA").decode() + EXTRA_TREES
    qs, trees = parse_trees(text)
    held = m.trees()
    sizes = [t["nodes"] for t in held]
    assert len(held) == len(trees) == 29 and 0 in sizes and 1 in sizes and max(sizes) >= 5
    deepest = held[int(np.argmax(sizes))]["name"]
    full = su.golden_bytes("full").decode().split()
    names = full + ["a-zz+b", "b-zz+a", "zz", "sil", "a-sil+b", "x-%s+y" % deepest, "e-%s+i" % deepest]
    tree, leaf = m.tree_descend(names, 2, 4)                                     # states 2 .. 5: nobody has a tree for state 5
    assert tree.shape == leaf.shape == (len(names), 4)
    for n, name in enumerate(names):
        base = name.split("-", 1)[-1].rsplit("+", 1)[0]
        for k in range(4):
            key = (base, 2 + k)
            if key not in trees:
                assert tree[n, k] == -1 and leaf[n, k] == -1, (name, key)
                continue
            t = held[tree[n, k]]
            assert (t["name"], t["state"]) == key
            assert t["leaves"][leaf[n, k]] == walk(qs, trees[key], name), (name, key)
    assert (tree[names.index("sil")] == -1).all() and (tree[:, 3] == -1).all() and (tree[names.index("zz"), :2] >= 0).all()
    ms = native.synth_last_kernel_ms()
    assert ms[0] > 0.0 and ms[1] > 0.0


def run_case(native, tmp_path, mmf_name, script, stats=None):
    from htk_amd import treeclust
    w = su.workdir(tmp_path, mmf_name)
    if stats:
        with open(os.path.join(w, "stats"), "wb") as f:
            f.write(open(stats, "rb").read())
    m = native.Mmf([os.path.join(w, "in.mmf")], hmm_list=os.path.join(w, "seen"))
    out = treeclust.run_script(m, treeclust.parse_script(script, synth=True), base_dir=w)
    m.write(m.packed(), one_file=os.path.join(w, "out.mmf"))
    return m, w, out


CASES = {"A": ("hmmdefs", None, "AU full\nCO tiedlist\nST trees\n"), "B": ("tied1.mmf", "LT treesA\n", "AU full\nCO tiedlist\nST trees\n"),
         "C": ("untied.mmf", None, "AU full\nCO tiedlist\n"), "D": ("mixD.mmf", "LT treesA\n", "AU full\nCO tiedlist\n")}


@pytest.mark.parametrize("case", sorted(CASES))
def test_cases_are_hhed_s_byte_for_byte(native, tmp_path, case):
    mmf_name, head, tail = CASES[case]
    m, w, out = run_case(native, tmp_path, mmf_name, (head or su.tb_script()) + tail)
    c = su.COUNTS["case" + case]
    (seen, unseen), (nlog, nphys) = out[-2], out[-1]
    assert (seen, seen + unseen, seen + unseen) == (c["AU"]["oldLog"], c["AU"]["log"], c["AU"]["phys"])
    assert (nlog, nphys) == (c["CO"]["logical"], c["CO"]["physical"]) == (len(m.logical), len(m.phys_names))
    su.same(open(os.path.join(w, "tiedlist"), "rb").read(), su.golden_bytes("tiedlist" + case), "tied list")
    su.same(open(os.path.join(w, "out.mmf"), "rb").read(), su.golden_bytes("synth%s.mmf" % case), "model set")
    if case == "A":
        assert open(os.path.join(w, "trees"), "rb").read() == su.golden_bytes("treesA")
    if case == "B":                                                                # ST after LT: the patterns turned, as with HHEd
        assert open(os.path.join(w, "trees"), "rb").read() == su.golden_bytes("treesA.lt_st")
        assert su.golden_bytes("tiedlistB") == su.golden_bytes("tiedlistA")         # LT restores what TB held
    if case == "C":
        assert nphys == 729                                                        # every synthesised model owns its matrix: nothing merges


def test_uncompacted_set_after_au_is_hhed_s(native, tmp_path):
    m, w, out = run_case(native, tmp_path, "hmmdefs", su.tb_script() + "AU full\n")
    assert m.logical_names == su.golden_bytes("full").decode().split() == m.phys_names      # SwapLists: the set's lists are the new list
    su.same(open(os.path.join(w, "out.mmf"), "rb").read(), su.golden_bytes("synthA_au.mmf"), "model set")


def test_case_e_is_refused_as_the_reference_fails(native, tmp_path):
    for trees, lst, key in (("treesA", "fullE", "caseE_error"), ("treesE2", "full", "caseE2_error")):
        d = tmp_path / key
        d.mkdir()
        with pytest.raises(native.HtkAmdError) as e:
            run_case(native, d, "tied1.mmf", "LT %s\nAU %s\n" % (trees, lst))
        mine = str(e.value).split("mmf_add_unseen: ")[-1]
        assert su.COUNTS[key].endswith(mine) and ("sil" in mine or "a-b+a state 4" in mine)


def test_live_against_hhed_with_other_occupations(native, tmp_path):
    if not os.path.exists(HHED):
        pytest.skip("oracle/_ref/HHEd is not built")
    mods = {}
    for name in ("make_treeclust_golden", "make_synth_golden"):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec); spec.loader.exec_module(mods[name])
    ref = tmp_path / "ref"; ref.mkdir(); mine = tmp_path / "mine"; mine.mkdir()
    w = su.workdir(ref, "hmmdefs")
    base = native.Mmf([os.path.join(w, "in.mmf")], hmm_list=os.path.join(w, "seen"))
    mods["make_treeclust_golden"].write_stats(base, os.path.join(w, "stats"), 23)
    assert open(os.path.join(w, "stats"), "rb").read() != tu.golden_bytes("stats")
    tail = "AU full\nCO tiedlist\nST trees\n"
    mods["make_synth_golden"].hhed(w, "in.mmf", "seen", mods["make_synth_golden"].tb_script() + tail, "out.mmf")
    _, w2, _ = run_case(native, mine, "hmmdefs", su.tb_script() + tail, stats=os.path.join(w, "stats"))
    for n in ("trees", "tiedlist", "out.mmf"):
        su.same(open(os.path.join(w2, n), "rb").read(), open(os.path.join(w, n), "rb").read(), n)
    assert open(os.path.join(w, "trees"), "rb").read() != su.golden_bytes("treesA")


def test_the_compacted_set_loads_and_resolves_an_unseen_triphone(native, tmp_path):
    m, w, _ = run_case(native, tmp_path, "hmmdefs", su.tb_script() + "AU full\nCO tiedlist\nST trees\n")
    seen = set(su.golden_bytes("seen").decode().split())
    name = [n for n in su.golden_bytes("full").decode().split() if n not in seen][0]
    qs, trees = parse_trees(su.golden_bytes("treesA").decode())
    base = name.split("-")[1].split("+")[0]
    want = [walk(qs, trees[(base, j)], name) for j in (2, 3, 4)]
    m2 = native.Mmf([os.path.join(w, "out.mmf")], hmm_list=os.path.join(w, "tiedlist"))
    pk = m2.packed()
    assert len(m2.logical) == 729 and pk["numPhys"] == su.COUNTS["caseA"]["CO"]["physical"]
    h = native.lib().htkamd_mmf_find_logical(m2.h, name.encode())
    assert h == m2.logical[name] and h >= 0
    off = pk["hmmStateOff"][h]
    assert [m2.state_macro(int(pk["hmmState"][off + j])) for j in range(3)] == want
    gm = native.Model(pk)                                                          # htkamd_model_create takes the set
    assert gm is not None
