"""MLLR mean transforms, the host side: which nodes get a transform (ParseNode), the transform file's writer and reader, the refusals --
against the reference's recorded run (tests/golden/mllr, tests/golden/make_mllr_golden.py).  No device is needed here."""
import json
import os
import subprocess

import numpy as np
import pytest

import regtree_util as ru
from htk_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mllr")
HEREST = os.path.join(ru.ROOT, "oracle", "_ref", "HERest")
REF = json.load(open(os.path.join(GOLDEN, "ref.json")))
KIDS = [tuple(k) for k in REF["children"]]
EINVAL, EMODEL = -1, -5


def _occ(case):
    """The occupations of the reference's trace.  Above the root it prints none (ParseTree returns first): the pass is the same, so `all`'s."""
    occ = REF["cases"][case]["nodeOcc"] or REF["cases"]["all"]["nodeOcc"]
    return [occ[str(n)] for n in range(1, len(KIDS) + 1)]


def _tree():
    kids = ru.parse_tree(open(os.path.join(GOLDEN, "rtree.tree")).read())
    classes = ru.parse_base(open(os.path.join(GOLDEN, "rtree.base")).read())
    term = [i + 1 for i, k in enumerate(kids) if k == (0, 0)]
    return capi.RegTree.from_tables(kids, dict(zip(term, classes)))


def _mmf(d=GOLDEN):
    return capi.Mmf([os.path.join(d, "hmmdefs")], hmm_list=os.path.join(d, "hmmlist"))


# ------------------------------------------------------------------------------------------ which nodes get a transform
def test_the_fixture_tree_has_seven_nodes():
    assert KIDS == [(2, 3), (4, 5), (6, 7), (0, 0), (0, 0), (0, 0), (0, 0)]


@pytest.mark.parametrize("case", ["all", "one", "subtree", "none", "equal", "equalBelow", "equalRoot"])
def test_node_selection_follows_the_reference(case):
    """The reference's node occupations (its trace) and threshold in, its numbering and class map (its transform file) out.  `equal`: the
    threshold is the occupation of terminal REF["equalNode"] as the trace prints it, which read back is the float itself; it counts as
    below (the strict >), so it and its smaller sibling share their parent's transform.  `equalBelow`, one float lower, gives it its own;
    `equalRoot`, the root on the threshold, gives no set."""
    ref = REF["cases"][case]
    if case == "equal":
        assert np.float32(ref["thresh"]) == np.float32(ref["nodeOcc"][str(REF["equalNode"])])
    rc, nodes, class_xform = capi.mllr_select(KIDS, _occ(case), ref["thresh"])
    assert class_xform == ref["classXform"] and len(nodes) == ref["numXforms"]
    assert rc == (capi.MLLR_NOSET if case in ("none", "equalRoot") else 0)
    # the nodes, read off ParseNode: post-order, a terminal below the threshold hands its class to the nearest ancestor above it
    small = REF["fallback"]["terminal"]
    parent = next(i + 1 for i, k in enumerate(KIDS) if small in k)
    one = [parent if n == small else n for n in (4, 5, 6, 7)]
    want = {"all": [4, 5, 6, 7], "one": one, "subtree": [3, 1], "none": [], "equal": [2, 6, 7], "equalBelow": one, "equalRoot": []}[case]
    assert nodes == want


def test_an_occupation_equal_to_the_threshold_counts_as_below():
    """node->nodeOcc > thresh is strict: further places of the tree than the recorded `equal` cases reach, on planted occupations."""
    occ = [1000.0, 400.0, 600.0, 150.0, 250.0, 300.0, 300.0]
    # terminal 4 sits exactly on it: its class waits while terminal 5 gets transform 1, then goes to the parent's transform 2
    assert capi.mllr_select(KIDS, occ, 150.0) == (0, [5, 2, 6, 7], [2, 1, 3, 4])
    assert capi.mllr_select(KIDS, occ, 149.99) == (0, [4, 5, 6, 7], [1, 2, 3, 4])
    assert capi.mllr_select(KIDS, occ, 400.0) == (0, [3, 1], [2, 2, 1, 1])             # inner node 2 on it: its classes to the root
    assert capi.mllr_select(KIDS, occ, 1000.0) == (capi.MLLR_NOSET, [], [0, 0, 0, 0])  # the root on it: no set
    assert capi.mllr_select(KIDS, occ, 600.0) == (0, [1], [1, 1, 1, 1])


def test_select_refuses_a_table_that_is_no_tree():
    with pytest.raises(capi.HtkAmdError) as e:
        capi.mllr_select([(2, 0), (0, 0)], [1.0, 1.0], 0.5)
    assert "node 1 has the children 2, 0" in str(e.value)


# ------------------------------------------------------------------------------------------ the file
@pytest.mark.parametrize("case", ["all", "one", "subtree", "none", "equal", "equalBelow", "equalRoot"])
def test_writer_gives_the_reference_file_back(case, tmp_path):
    src = os.path.join(GOLDEN, "xf_" + case, "sp1.mllr")
    x = capi.Mllr.read(src)
    ref = REF["cases"][case]
    assert x.num_xforms == ref["numXforms"] and x.class_xform == ref["classXform"]
    if x.num_xforms:
        assert x.blocks == REF["blocks"] and x.vec_size == sum(REF["blocks"])
        A, b = x.xform(1)
        assert b is not None and A[0, 2] == 0.0 and A[2, 0] == 0.0 and A[0, 0] != 0.0
    x.write(tmp_path / "out.mllr")
    assert open(tmp_path / "out.mllr", "rb").read() == open(src, "rb").read()


def test_from_tables_writes_the_same_bytes(tmp_path):
    src = os.path.join(GOLDEN, "xf_one", "sp1.mllr")
    x = capi.Mllr.read(src)
    mats = [x.xform(k) for k in range(1, x.num_xforms + 1)]
    y = capi.Mllr.from_tables(np.array([m[0] for m in mats]), np.array([m[1] for m in mats]), x.class_xform, blocks=REF["blocks"], name="sp1.mllr")
    y.write(tmp_path / "y.mllr")
    assert open(tmp_path / "y.mllr", "rb").read() == open(src, "rb").read()


REFUSED = [
    ("<XFORMSET>", '<PARENTXFORM>~a "parent"\n<XFORMSET>', "<PARENTXFORM>"),
    ("<XFORMKIND>MLLRMEAN", "<XFORMKIND>CMLLR", "<XFORMKIND> CMLLR"),
    ("<XFORMKIND>MLLRMEAN", "<XFORMKIND>MLLRCOV", "<XFORMKIND> MLLRCOV"),
    ("<XFORMKIND>MLLRMEAN", "<XFORMKIND>SEMIT", "<XFORMKIND> SEMIT"),
    ("<ADAPTKIND>TREE", "<ADAPTKIND>BASE", "<ADAPTKIND> BASE"),
]


@pytest.mark.parametrize("old, new, name", REFUSED)
def test_reader_refuses_what_is_out_of_scope_by_name(old, new, name, tmp_path):
    text = open(os.path.join(GOLDEN, "xf_one", "sp1.mllr")).read()
    assert old in text
    (tmp_path / "bad.mllr").write_text(text.replace(old, new, 1))
    with pytest.raises(capi.HtkAmdError) as e:
        capi.Mllr.read(tmp_path / "bad.mllr")
    assert name in str(e.value) and "not supported" in str(e.value) and e.value.rc == EINVAL


def test_reader_refuses_a_binary_file(tmp_path):
    (tmp_path / "bin.mllr").write_bytes(b'~a "x"\n\x00\x5a\x00\x00')
    with pytest.raises(capi.HtkAmdError) as e:
        capi.Mllr.read(tmp_path / "bin.mllr")
    assert "only the text form" in str(e.value)


@pytest.mark.skipif(not os.path.exists(HEREST), reason="oracle/_ref/HERest is not built (the reference is not on this machine)")
def test_the_reference_reads_our_file(tmp_path):
    """A file we wrote, as the input transform (-a -J) of a reference pass over the speaker's data."""
    xf = tmp_path / "xf"
    xf.mkdir()
    capi.Mllr.read(os.path.join(GOLDEN, "xf_one", "sp1.mllr")).write(xf / "sp1.mllr")
    (tmp_path / "out").mkdir()
    r = subprocess.run([HEREST, "-C", "config", "-S", "train.scp", "-I", "labels.mlf", "-H", "hmmdefs", "-u", "m", "-a", "-J", str(xf), "mllr", "-J", ".",
                        "-h", "*/%%%_*", "-M", str(tmp_path / "out"), "hmmlist"], cwd=GOLDEN, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stdout, r.stdout[-2000:]
    assert os.path.exists(tmp_path / "out" / "hmmdefs")


# ------------------------------------------------------------------------------------------ refusals, before a device is looked for
HDR = "~o <STREAMINFO> 1 2 <VECSIZE> 2 <NULLD><USER>%s\n"
TRANS = "<TRANSP> 3\n0 1 0\n0 .5 .5\n0 0 0\n<ENDHMM>\n"
VAR = "<VARIANCE> 2\n1 1\n"
ONE = "<MEAN> 2\n0 0\n" + VAR


def _hmm(name, body):
    return '~h "%s"\n<BEGINHMM>\n<NUMSTATES> 3\n<STATE> 2\n%s%s' % (name, body, TRANS)


EXCLUDED = {
    "streams": ("~o <STREAMINFO> 2 1 1 <VECSIZE> 2 <NULLD><USER><DIAGC>\n" +
                _hmm("a", "<STREAM> 1\n<MEAN> 1\n0\n<VARIANCE> 1\n1\n<STREAM> 2\n<MEAN> 1\n0\n<VARIANCE> 1\n1\n"), "a set with more than one stream (2) is not supported"),
    "fullc": (HDR % "<FULLC>" + _hmm("a", "<MEAN> 2\n0 0\n<INVCOVAR> 2\n2 0.5\n1\n"), "FULLC sets are not supported"),
    "tiedmix": (HDR % "<DIAGC>" + '~m "TM_1_1"\n' + ONE + '~m "TM_1_2"\n<MEAN> 2\n1 1\n' + VAR + _hmm("a", '<NUMMIXES> 2\n<TMIX> "TM_1_"\n 0.5 0.5\n'),
                "tied-mixture sets are not supported"),
    "sharedmean": (HDR % "<DIAGC>" + '~u "mu1"\n<MEAN> 2\n0 0\n' + _hmm("a", '<NUMMIXES> 2\n<MIXTURE> 1 0.5\n~u "mu1"\n' + VAR + '<MIXTURE> 2 0.5\n~u "mu1"\n<VARIANCE> 2\n2 2\n'), "sets with shared mean vectors (~u) are not supported"),
    "discrete": (HDR.replace("<USER>", "<DISCRETE>") % "<DIAGC>" + _hmm("a", ONE), "discrete sets are not supported"),
}


def _both(mmf, tree, message, rc, **cfg):
    """mllr_check refuses with the message; mllr_estimate (no model, no statistics: it must not get that far) with the same reason."""
    with pytest.raises(capi.HtkAmdError) as e:
        capi.Mllr.check(mmf, tree, **cfg)
    assert str(e.value) == "mllr_check failed (%d): mllr_check: %s" % (rc, message)
    with pytest.raises(capi.HtkAmdError) as e:
        capi.Mllr.estimate(mmf, None, None, tree, **cfg)
    assert str(e.value) == "mllr_estimate failed (%d): mllr_estimate: %s" % (rc, message)


@pytest.mark.parametrize("kind", sorted(EXCLUDED))
def test_check_refuses_excluded_sets_by_name(kind, tmp_path):
    text, message = EXCLUDED[kind]
    (tmp_path / "hmmdefs").write_text(text)
    (tmp_path / "hmmlist").write_text("a\n")
    tree = capi.RegTree.from_tables([(0, 0)], {1: [("a", 2, 1)]})
    _both(_mmf(str(tmp_path)), tree, message, EMODEL)


def test_check_refuses_blocks_that_do_not_sum_to_the_vector_size():
    _both(_mmf(), _tree(), "BLOCKSIZE: the blocks sum to 5, the vector size is 6", EINVAL, blocks=[2, 3])
    _both(_mmf(), _tree(), "BLOCKSIZE: block 2 has size 0", EINVAL, blocks=[6, 0])


def test_check_refuses_a_missing_tree():
    _both(_mmf(), None, "ADAPTKIND = BASE (no regression class tree) is not supported", EINVAL)


@pytest.mark.parametrize("comp, why", [(("nomodel", 2, 1), "the set has no model nomodel"), (("m00", 5, 1), "the model has the emitting states 2 .. 4"),
                                       (("m00", 2, 3), "the state has 2 mixture components")])
def test_check_refuses_a_tree_with_a_component_outside_the_set(comp, why):
    tree = capi.RegTree.from_tables([(2, 3), (0, 0), (0, 0)], {2: [("m01", 2, 1)], 3: [("m02", 3, 2), comp]})
    _both(_mmf(), tree, "the tree's component %s.state[%d].mix[%d] (class 2): %s" % (comp + (why,)), EMODEL)


def test_check_passes_the_fixture_and_maps_every_gaussian():
    mmf, tree = _mmf(), _tree()
    capi.Mllr.check(mmf, tree, blocks=REF["blocks"])
    cls = capi.Mllr.gauss_classes(mmf, tree)
    assert cls.min() == 1 and cls.max() == 4 and len(cls) == 8 * 3 * 2
