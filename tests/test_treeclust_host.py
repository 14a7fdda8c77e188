"""Decision-tree state clustering, the host side (htk_amd/host/treeclust.c): the statistics reader, item lists and questions against
what the reference's HHEd printed for the fixture (tests/golden/make_treeclust_golden.py), the trees-file writer, and every refusal with
its reason.  The clustering itself runs on the device: tests/test_gpu_treeclust.py."""
import json
import os

import numpy as np
import pytest

import treeclust_util as tu
from treeclust_util import G

EMODEL = -5                                                          # HTKAMD_EMODEL
HDR = "~o <STREAMINFO> 1 2 <VECSIZE> 2 <NULLD><USER>%s\n"
TRANS = "<TRANSP> 3\n0 1 0\n0 .5 .5\n0 0 0\n<ENDHMM>\n"
VAR = "<VARIANCE> 2\n1 1\n"
ONE = "<MEAN> 2\n0 0\n" + VAR


def hmm(name, body):
    return '~h "%s"\n<BEGINHMM>\n<NUMSTATES> 3\n<STATE> 2\n%s%s' % (name, body, TRANS)


@pytest.fixture()
def fixture_set(native, tmp_path):
    mmf_path, lst = tu.unpack_inputs(tmp_path)
    return native.Mmf([mmf_path], hmm_list=lst)


def small_set(native, tmp_path, text, name="set"):
    p = tmp_path / name
    p.write_text(text)
    return native.Mmf(files=[str(p)])


def test_stats_reader_against_the_fixture_and_round_trip(native, fixture_set, tmp_path):
    m = fixture_set
    occ, cnt = native.read_stats(m, os.path.join(G, "stats"))
    pk = m.packed()
    assert occ.shape == (pk["numStates"],) and cnt.shape == (pk["numPhys"],)
    # the file's own numbers, line by line: index, "name", count, three occupations
    seen = 0
    for line in open(os.path.join(G, "stats")):
        f = line.split()
        h = m.phys_names.index(f[1].strip('"'))
        assert cnt[h] == int(f[2])
        st = pk["hmmState"][pk["hmmStateOff"][h]:pk["hmmStateOff"][h + 1]]
        assert [np.float32(x) for x in f[3:]] == list(occ[st])
        seen += 1
    assert seen == pk["numPhys"] and (occ == 0).sum() >= 7 and (occ > 0).sum() > 400
    # write what was read, read it again
    lay = native.accs_layout(pk)
    vec = np.zeros(lay.total)
    vec[lay.wtOcc:lay.wtOcc + pk["numStates"]] = occ
    vec[lay.nEgs:lay.nEgs + pk["numPhys"]] = cnt
    native.stats_write_file(pk, vec, m.phys_names, str(tmp_path / "again"))
    assert open(tmp_path / "again").read() == open(os.path.join(G, "stats")).read()
    occ2, cnt2 = native.read_stats(m, str(tmp_path / "again"))
    assert np.array_equal(occ, occ2) and np.array_equal(cnt, cnt2)


def test_stats_reader_refusals(native, fixture_set, tmp_path):
    lines = open(os.path.join(G, "stats")).read().splitlines()
    (tmp_path / "unknown").write_text(lines[0] + "\n" + '   2  "q-q+q"    3    1.0 2.0 3.0\n')
    with pytest.raises(native.HtkAmdError, match="unknown model q-q\\+q at line 2"):
        native.read_stats(fixture_set, str(tmp_path / "unknown"))
    (tmp_path / "short").write_text(" ".join(lines[0].split()[:-1]) + "\n")
    with pytest.raises(native.HtkAmdError, match="2 occupation counts for model .* which has 3 emitting states"):
        native.read_stats(fixture_set, str(tmp_path / "short"))
    with pytest.raises(native.HtkAmdError, match="cannot open"):
        native.read_stats(fixture_set, str(tmp_path / "absent"))


def test_item_list_order_and_question_answers_as_hhed_sees_them(native, fixture_set):
    probe = json.load(open(os.path.join(G, "probe.json")))
    m = fixture_set
    items = m.item_list(probe["item_list"])
    # PState prints the models it walks and prepends each: the list is what it printed, backwards
    assert [m.phys_names[h] for h, _ in items] == probe["pstate_walk"][::-1]
    assert {j for _, j in items} == {3} and len(items) == 91
    # two sets: the later one stands in front
    a = m.item_list('{("*-b+*").state[3]}'); b = m.item_list('{("*-a+*").state[3]}')
    assert m.item_list('{*-a+*.state[3],*-b+*.state[3]}') == a + b
    ans = m.question_answers("L_Stop", probe["question"])
    assert sorted(n for n, x in zip(m.phys_names, ans) if x) == probe["answers_true"]
    assert not m.question_answers("none", ["z-*"]).any()
    assert m.question_answers("one", ["a-a+a"]).sum() == 1           # a full name is looked up, not matched


def test_trees_writer_on_a_hand_built_tree(native, tmp_path):
    q = [("L_Nasal", ["m-*", "n-*"]), ("R_a", ["*+a"])]
    t = [dict(name="aa", state=2, quest=[0, 1], no=[-3, -2], yes=[1, -1], leaves=["ST_aa_2_1", "ST_aa_2_2", "ST_aa_2_3"]),
         dict(name="sil", state=3, quest=[], no=[], yes=[], leaves=["ST_sil_3_1"])]
    native.trees_write(str(tmp_path / "trees"), q, t)
    assert open(tmp_path / "trees").read() == open(os.path.join(G, "trees_hand.expected")).read()


def cluster(native, m, specs, questions=(("L_a", ["a-*"]),), occ="ones", **kw):
    if isinstance(occ, str):
        occ = np.ones(m.desc.numStates, np.float32)
    return m.tree_cluster(occ, list(questions), specs, **kw)


@pytest.mark.parametrize("items,reason", [
    ("{*-a+*}", "whole models"),
    ("{*-a+*.transP}", "only .state\\[i\\] items"),
    ("{*-a+*.state[2].mix[1]}", "items below the state"),
    ("{*-a+*.state[2].stream[1].mix[1]}", "items below the state"),
    ("{*-a+*.state[2-4]}", "index range"),
    ("{*-a+*.state[2,3]}", "index range"),
    ("{*-z+*.state[2]}", "no items to cluster"),
    ("*-a+*.state[2]", "{ expected"),
])
def test_item_lists_that_are_refused(native, fixture_set, items, reason):
    with pytest.raises(native.HtkAmdError, match=reason) as e:
        cluster(native, fixture_set, [(10.0, "X_", items)])
    assert e.value.rc == -1                                          # HTKAMD_EINVAL


def test_calls_that_are_refused(native, fixture_set, tmp_path):
    m = fixture_set
    with pytest.raises(native.HtkAmdError, match="question name L_a invalid"):
        cluster(native, m, [(10.0, "X_", "{*-a+*.state[2]}")], questions=[("L_a", ["a-*"]), ("L_b", ["b-*"]), ("L_a", ["c-*"])])
    with pytest.raises(native.HtkAmdError, match="selected twice \\(by X_ and Y_\\): trees must not overlap"):
        cluster(native, m, [(10.0, "X_", "{*-a+*.state[2]}"), (10.0, "Y_", "{a-a+*.state[2]}")])
    L, C = native.lib(), native.C
    spec = (native.TreeSpec * 1)(native.TreeSpec(10.0, b"X_", b"{*-a+*.state[2]}"))
    rc = L.htkamd_mmf_tree_cluster(m.h, None, C.c_float(-1.0), None, 0, spec, 1, 3, None, None)
    assert rc == -1 and b"no stats loaded" in L.htkamd_last_error()
    from htk_amd import treeclust
    with pytest.raises(native.HtkAmdError, match="no stats loaded"):
        treeclust.run_script(m, treeclust.parse_script('TB 10.0 "X_" {*-a+*.state[2]}\n'))
    with pytest.raises(native.HtkAmdError, match="command MU is not supported"):
        treeclust.parse_script("RO 10 stats\nMU 2 {*.state[2-4].mix}\n")


def test_model_sets_that_are_refused(native, tmp_path):
    two = "<NUMMIXES> 2\n<MIXTURE> 1 0.5\n" + ONE + "<MIXTURE> 2 0.5\n<MEAN> 2\n1 1\n" + VAR
    sets = {
        "mixtures": (HDR % "<DIAGC>" + hmm("a", two), "has 2 mixture components: TB only valid for 1 mix diagonal covar models"),
        "fullc": (HDR % "<FULLC>" + hmm("a", "<MEAN> 2\n0 0\n<INVCOVAR> 2\n2 0.5\n1\n"), "FULLC sets are not supported"),
        "streams": ("~o <STREAMINFO> 2 1 1 <VECSIZE> 2 <NULLD><USER><DIAGC>\n" +
                    hmm("a", "<STREAM> 1\n<MEAN> 1\n0\n<VARIANCE> 1\n1\n<STREAM> 2\n<MEAN> 1\n0\n<VARIANCE> 1\n1\n"), "more than one stream"),
        "tiedmix": (HDR % "<DIAGC>" + '~m "TM_1_1"\n' + ONE + '~m "TM_1_2"\n<MEAN> 2\n1 1\n' + VAR + hmm("a", '<NUMMIXES> 2\n<TMIX> "TM_1_"\n 0.5 0.5\n'),
                    "tied-mixture sets are not supported"),
        "tied_already": (HDR % "<DIAGC>" + '~s "s1"\n' + ONE + hmm("a", '~s "s1"\n'), "is the ~s macro s1 already"),
    }
    for name, (text, reason) in sets.items():
        m = small_set(native, tmp_path, text, name)
        with pytest.raises(native.HtkAmdError, match=reason) as e:
            cluster(native, m, [(10.0, "X_", "{a.state[2]}")], questions=[("Q", ["a"])])
        assert e.value.rc == EMODEL, name


def test_tree_cluster_fails_loudly_without_a_device(native, fixture_set):
    if native.lib().htkamd_device_count() > 0:
        pytest.skip("a GPU is present")
    occ, _ = native.read_stats(fixture_set, os.path.join(G, "stats"))
    with pytest.raises(native.HtkAmdError, match="no HIP device"):
        fixture_set.tree_cluster(occ, [("L_a", ["a-*"])], [(10.0, "X_", "{*-a+*.state[2]}")])
    with pytest.raises(native.HtkAmdError, match="no HIP device"):
        native.tree_split_sums(np.ones((3, 3), np.float32), [0, 1, 2], np.ones((1, 3), np.uint8))
