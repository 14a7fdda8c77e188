"""Regression class trees (HHEd RC), the host side: the edit-script parser, the refusals, the two writers and the order of the member
list -- against HHEd's recorded files (tests/golden/regtree, tests/golden/make_regtree_golden.py).  No device is needed here."""
import ctypes as C
import os

import numpy as np
import pytest

import regtree_util as ru
from htk_amd import capi, treeclust

EMODEL = -5

CASES = sorted(ru.CASES)


def _golden(name, f):
    return open(os.path.join(ru.GOLDEN, name, f), "rb").read()


# ------------------------------------------------------------------------------------------ the edit script
def test_parser_takes_rc_only_when_asked():
    sc = treeclust.parse_script('LS stats\nRC 4 "rtree" {sil.state[2-4].mix}\nRC 16 cls\n', regtree=True)
    assert sc.commands == [("LS", "stats"), ("RC", 4, "rtree", "{sil.state[2-4].mix}"), ("RC", 16, "cls", None)]
    sc = treeclust.parse_script('RC 2 "my tree" {sil.state[2].mix}\nRC 3 \'a b\'\nRC 4 "q\\"x"{*.state[2].mix}\n', regtree=True)      # a quoted identifier as ChkedAlpha reads it
    assert sc.commands == [("RC", 2, "my tree", "{sil.state[2].mix}"), ("RC", 3, "a b", None), ("RC", 4, 'q"x', "{*.state[2].mix}")]
    with pytest.raises(capi.HtkAmdError) as e:
        treeclust.parse_script("RC 4 rtree\n")
    assert str(e.value) == "edit script: command RC is not supported (only RO, TR, QS, TB, ST, TC, NC, TI, LS: state clustering and tying)"
    with pytest.raises(capi.HtkAmdError) as e:
        treeclust.parse_script("RC 4 rtree\n", synth=True)
    assert "command RC is not supported" in str(e.value)


@pytest.mark.parametrize("line, why", [("RC 4", "identifier expected"), ("RC x rtree", "identifier expected"), ("RC 257 rtree", "256"),
                                       ("RC -1 rtree", "256"), ("RC 4 rtree sil", "item list")])
def test_parser_refuses_bad_rc(line, why):
    with pytest.raises(capi.HtkAmdError) as e:
        treeclust.parse_script(line + "\n", regtree=True)
    assert why in str(e.value)


def test_runner_wants_statistics_before_rc():
    d = os.path.join(ru.GOLDEN, "a")
    mmf = capi.Mmf([os.path.join(d, "hmmdefs")], hmm_list=os.path.join(d, "hmmlist"))
    with pytest.raises(capi.HtkAmdError) as e:
        treeclust.run_script(mmf, treeclust.parse_script("RC 1 rtree\n", regtree=True))
    assert "no stats loaded" in str(e.value)


# ------------------------------------------------------------------------------------------ refusals, by name, before a device is touched
HDR = "~o <STREAMINFO> 1 2 <VECSIZE> 2 <NULLD><USER>%s\n"
TRANS = "<TRANSP> 3\n0 1 0\n0 .5 .5\n0 0 0\n<ENDHMM>\n"
VAR = "<VARIANCE> 2\n1 1\n"
ONE = "<MEAN> 2\n0 0\n" + VAR


def _hmm(name, body):
    return '~h "%s"\n<BEGINHMM>\n<NUMSTATES> 3\n<STATE> 2\n%s%s' % (name, body, TRANS)


EXCLUDED = {
    "streams": ("~o <STREAMINFO> 2 1 1 <VECSIZE> 2 <NULLD><USER><DIAGC>\n" +
                _hmm("a", "<STREAM> 1\n<MEAN> 1\n0\n<VARIANCE> 1\n1\n<STREAM> 2\n<MEAN> 1\n0\n<VARIANCE> 1\n1\n"),
                "mmf_regtree: a set with more than one stream (2) is not supported"),
    "fullc": (HDR % "<FULLC>" + _hmm("a", "<MEAN> 2\n0 0\n<INVCOVAR> 2\n2 0.5\n1\n"), "mmf_regtree: FULLC sets are not supported"),
    "tiedmix": (HDR % "<DIAGC>" + '~m "TM_1_1"\n' + ONE + '~m "TM_1_2"\n<MEAN> 2\n1 1\n' + VAR + _hmm("a", '<NUMMIXES> 2\n<TMIX> "TM_1_"\n 0.5 0.5\n'),
                "mmf_regtree: tied-mixture sets are not supported"),
    "discrete": (HDR.replace("<USER>", "<DISCRETE>") % "<DIAGC>" + _hmm("a", ONE), "mmf_regtree: discrete sets are not supported"),
}


@pytest.mark.parametrize("kind", sorted(EXCLUDED))
def test_refuses_excluded_sets_by_name(kind, tmp_path):
    """Multi-stream, FULLC, tied-mixture and discrete sets, each written here as text: the call names the kind and says EMODEL; with more
    than one terminal asked for, so the refusal is what keeps the call from the device."""
    import numpy as np
    text, message = EXCLUDED[kind]
    p = tmp_path / kind
    p.write_text(text)
    m = capi.Mmf([str(p)])
    with pytest.raises(capi.HtkAmdError) as e:
        m.regtree(np.ones(m.desc.numStates, np.float32), 4)
    assert message in str(e.value) and str(e.value).startswith("mmf_regtree failed")
    assert e.value.rc == EMODEL


@pytest.mark.parametrize("items, why", [("{m00.state[2]}", "whole states"), ("{m00}", "whole models"), ("{m00.transP}", "state expected"),
                                        ("{m00.state[2].mix[1]}", "mixture components"), ("{m00.state[2].dur}", "only hname.state[i-j].mix"),
                                        ("{m00.state[9].mix}", "out of range"),
                                        ("{*.state[2-4].mix}", "every Gaussian")])
def test_refuses_item_lists_that_are_not_pdfs(items, why):
    import numpy as np
    d = os.path.join(ru.GOLDEN, "a")
    mmf = capi.Mmf([os.path.join(d, "hmmdefs")], hmm_list=os.path.join(d, "hmmlist"))
    with pytest.raises(capi.HtkAmdError) as e:
        mmf.regtree(np.ones(mmf.desc.numStates, np.float32), 4, items)
    assert why in str(e.value)


def test_refuses_bad_terminal_counts_and_identifiers(tmp_path):
    import numpy as np
    d = os.path.join(ru.GOLDEN, "a")
    mmf = capi.Mmf([os.path.join(d, "hmmdefs")], hmm_list=os.path.join(d, "hmmlist"))
    with pytest.raises(capi.HtkAmdError):
        mmf.regtree(np.ones(mmf.desc.numStates, np.float32), 257)
    t = mmf.regtree(np.ones(mmf.desc.numStates, np.float32), 1)
    for ident in ("a/b", "a.tree", ""):
        with pytest.raises(capi.HtkAmdError):
            t.write(ident, str(tmp_path))


# ------------------------------------------------------------------------------------------ the writers
FILES = [(c, ru.IDENT) for c in CASES] + sorted(ru.NO_SPLIT)      # (case directory, identifier): every pair of files HHEd recorded


@pytest.mark.parametrize("name, ident", FILES)
def test_writers_give_hhed_bytes_from_tables(name, ident, tmp_path):
    kids = ru.parse_tree(_golden(name, ident + ".tree").decode())
    classes = ru.parse_base(_golden(name, ident + ".base").decode())
    terms = [i + 1 for i, k in enumerate(kids) if k == (0, 0)]
    t = capi.RegTree.from_tables(kids, dict(zip(terms, classes)))
    assert t.num_nodes == len(kids) and t.num_terminals == len(terms)
    assert [t.children(i + 1) for i in range(len(kids))] == kids
    assert [t.terminal_node(k + 1) for k in range(len(terms))] == terms and t.terminal_node(len(terms) + 1) == 0
    assert [t.components(n) for n in terms] == classes
    t.write(ident, str(tmp_path))
    assert (tmp_path / (ident + ".tree")).read_bytes() == _golden(name, ident + ".tree")
    assert (tmp_path / (ident + ".base")).read_bytes() == _golden(name, ident + ".base")


def test_writer_takes_classes_that_interleave_many_models(tmp_path):
    """Every class walks through every model (what a deep tree over a large set looks like): the names are found by hash, whatever the order."""
    H, K = 3000, 4
    classes = [[("m%04d" % h, 2 + k % 3, 1 + k) for h in range(H)] for k in range(K)]
    kids = [(2, 3), (4, 5), (6, 7), (0, 0), (0, 0), (0, 0), (0, 0)]
    t = capi.RegTree.from_tables(kids, dict(zip((4, 5, 6, 7), classes)))
    assert [t.components(n) for n in (4, 5, 6, 7)] == classes
    t.write("big", str(tmp_path))
    assert ru.parse_base((tmp_path / "big.base").read_text()) == classes


def test_from_tables_refuses_what_is_no_tree():
    for kids in ([(2, 3), (0, 0)], [(2, 2), (0, 0), (0, 0)], [(0, 0), (0, 0)], [(2, 3), (1, 3), (0, 0)]):
        with pytest.raises(capi.HtkAmdError):
            capi.RegTree.from_tables(kids, {})


# ------------------------------------------------------------------------------------------ the member list
@pytest.mark.parametrize("name, ident", sorted(ru.NO_SPLIT))
def test_unsplit_lists_are_hhed_bytes(name, ident, tmp_path):
    """RC 1 (RC 2 behind a non-speech list) splits nothing: the files hold InitRegTree's lists as the scan made them, and no device is used.
    (c, items): the list in every form the parser takes -- a parenthesised model list, quoted names, patterns, an index list, several
    items -- gives the two classes HHEd's own parser gave."""
    t = ru.run_library(os.path.join(ru.GOLDEN, name), tmp_path, script=ident + ".hed")
    assert t.stats() == ([], 0.0)
    assert (tmp_path / (ident + ".tree")).read_bytes() == _golden(name, ident + ".tree")
    assert (tmp_path / (ident + ".base")).read_bytes() == _golden(name, ident + ".base")


def test_item_list_forms_select_what_the_plain_list_selects():
    d = os.path.join(ru.GOLDEN, "c")
    mmf = capi.Mmf([os.path.join(d, "hmmdefs")], hmm_list=os.path.join(d, "hmmlist"))
    occ, _ = capi.read_stats(mmf, os.path.join(d, "stats"))
    forms, plain = mmf.regtree(occ, 2, ru.NO_SPLIT[("c", "items")][1]), mmf.regtree(occ, 2, ru.ITEMS_PLAIN)
    assert forms.components(2) == plain.components(2) and forms.components(3) == plain.components(3)
    assert len(forms.components(2)) == 28 and len(forms.components(3)) == 8
    assert forms.components(2) == ru.parse_base(_golden("c", "items.base").decode())[0]
    with pytest.raises(capi.HtkAmdError) as e:
        mmf.regtree(occ, 2, "{(sil,m01.state[2].mix}")
    assert ") expected" in str(e.value)
    with pytest.raises(capi.HtkAmdError) as e:
        mmf.regtree(occ, 2, '{"sil.state[2].mix}')
    assert "unterminated quote" in str(e.value)


@pytest.mark.parametrize("name", CASES)
def test_member_order_against_the_golden_base(name, tmp_path):
    """A split keeps the list's order inside each child, so every class of HHEd's base file is a subsequence of the scan's list -- which the
    library gives without a device when nothing is split -- and together the classes are that list."""
    d = os.path.join(ru.GOLDEN, name)
    mmf = capi.Mmf([os.path.join(d, "hmmdefs")], hmm_list=os.path.join(d, "hmmlist"))
    occ, _ = capi.read_stats(mmf, os.path.join(d, "stats"))
    items = ru.CASES[name][2]
    t = mmf.regtree(occ, 2 if items else 1, items)
    members = [c for k in range(t.num_terminals) for c in t.components(t.terminal_node(k + 1))]
    classes = ru.parse_base(_golden(name, "rtree.base").decode())
    assert sorted(members) == sorted(c for cl in classes for c in cl) and len(set(members)) == len(members)
    place = {c: i for i, c in enumerate(members)}
    for cl in classes:
        pos = [place[c] for c in cl]
        assert pos == sorted(pos)
    if items:
        assert classes[0] == t.components(2)


# ------------------------------------------------------------------------------------------ the test aid over the device steps
def test_probe_refuses_before_a_device_is_touched():
    """capi.regtree_probe (htkamd_regtree_probe): a step of an unknown kind, a vector size above 960 and arrays that do not fit are
    refused by name; without a device the call fails loudly, as every entry point does."""
    z = lambda n, D: (np.zeros((n, D), np.float32),) * 3 + (np.zeros(n, np.float32), np.ones(n, np.uint8))
    with pytest.raises(capi.HtkAmdError) as e:
        capi.regtree_probe(*z(4, 3), [("merge", 0, 4)])
    assert "step 0" in str(e.value)
    steps = np.array([[2, 0, 4]], np.int32)
    out = np.zeros(64, np.float32)
    a = z(4, 3)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert capi.lib().htkamd_regtree_probe(p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(a[4]), 4, 3, p(steps), p(out), 1, p(steps.copy()), p(out), p(steps.copy()), None) == -1
    assert b"kind 2" in capi.lib().htkamd_last_error()
    assert capi.lib().htkamd_regtree_probe(p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(a[4]), 4, 3, None, p(out), 0, None, p(out), None, None) == -1
    with pytest.raises(capi.HtkAmdError) as e:
        capi.regtree_probe(*z(2, 961), [("node", 0, 2)])
    assert "bad argument" in str(e.value)
    with pytest.raises(capi.HtkAmdError) as e:
        capi.regtree_probe(np.zeros((4, 3)), np.zeros((4, 2)), np.zeros((4, 3)), np.zeros(4), np.ones(4), [])
    assert "bad shapes" in str(e.value)
    if capi.lib().htkamd_device_count() == 0:
        with pytest.raises(capi.HtkAmdError) as e:
            capi.regtree_probe(*z(4, 3), [("node", 0, 4)])
        assert "no HIP device" in str(e.value)
