"""Data-driven state clustering (HHEd TC / NC / TI), the parts that need no device: script parsing and order, every refusal by reason
and return code, TI byte for byte against the reference's output (tests/golden/datacluster, script d), the no-device error."""
import os

import numpy as np
import pytest

import datacluster_util as du
import treeclust_util as tu

EINVAL, ENODEV, EMODEL = -1, -2, -5
GOLD = os.path.join(tu.ROOT, "tests", "golden")


@pytest.fixture()
def fixture_set(native, tmp_path):
    mmf, lst = tu.unpack_inputs(tmp_path)
    return native.Mmf([mmf], hmm_list=lst)


def load_sub(native, tmp_path, name):
    import re
    text = du.golden_bytes(name)
    p, lst = tmp_path / name, tmp_path / "sublist"
    p.write_bytes(text)
    lst.write_text("\n".join(re.findall(r'^~h "([^"]+)"', text.decode(), flags=re.M)) + "\n")
    return native.Mmf([str(p)], hmm_list=str(lst))


def test_new_commands_parse_and_keep_script_order(native):
    from htk_amd import treeclust
    sc = treeclust.parse_script('RO 60.0 stats\nTC 0.90 "A_" {("*-a+*").state[2]}\nQS \'L_a\' { "a-*" }\nTB 12.0 "B_" {*-b+*.state[2]}\n'
                                'NC 4 "C_" {*-c+*.state[3]}\nLS other\nTI "T_x" {(*-b+*,*-c+*).transP}\nST trees\n')
    assert [c[0] for c in sc.commands] == ["RO", "TC", "QS", "TB", "NC", "LS", "TI", "ST"]
    assert sc.commands[1] == ("TC", 0.9, "A_", '{("*-a+*").state[2]}')
    assert sc.commands[4] == ("NC", 4, "C_", "{*-c+*.state[3]}")
    assert sc.commands[5] == ("LS", "other") and sc.commands[6] == ("TI", "T_x", "{(*-b+*,*-c+*).transP}")
    assert sc.specs == [(12.0, "B_", "{*-b+*.state[2]}")] and sc.outlier == 60.0 and sc.trees_path == "trees"
    with pytest.raises(native.HtkAmdError, match="command MU is not supported"):
        treeclust.parse_script("TC 1.0 X_ {*.state[2]}\nMU 2 {*.state[2-4].mix}\n")
    for cmd in ("AU list", "LT trees", "CO list"):
        with pytest.raises(native.HtkAmdError, match="command %s is not supported" % cmd[:2]):
            treeclust.parse_script(cmd + "\n")


def test_a_script_without_tb_is_legal_and_fails_at_the_device_only(native, fixture_set):
    from htk_amd import treeclust
    if native.lib().htkamd_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(native.HtkAmdError, match="no HIP device"):
        treeclust.run_script(fixture_set, treeclust.parse_script('TC 0.9 "A_" {*-a+*.state[2]}\n'))


@pytest.mark.parametrize("items,reason", [
    ("{*-a+*.transP}", "only .state\\[i\\] items are clustered"),
    ("{*-a+*}", "whole models"),
    ("{*-a+*.state[2].mix[1]}", "items below the state"),
    ("{*-a+*.state[2-4]}", "an index range"),
])
def test_items_that_are_not_single_states_are_refused(native, fixture_set, items, reason):
    with pytest.raises(native.HtkAmdError, match=reason) as e:
        fixture_set.data_cluster(None, [("TC", 1.0, "X_", items)])
    assert e.value.rc == EINVAL


def test_refusals_by_reason_and_code(native, fixture_set, tmp_path):
    m = fixture_set
    with pytest.raises(native.HtkAmdError, match="selected twice \\(by X_ and Y_\\): commands must not overlap") as e:
        m.data_cluster(None, [("TC", 1.0, "X_", "{*-a+*.state[2]}"), ("NC", 2, "Y_", "{a-a+*.state[2]}")])
    assert e.value.rc == EINVAL
    with pytest.raises(native.HtkAmdError, match="rather long for a macro name") as e:
        m.data_cluster(None, [("TC", 1.0, "X" * 21, "{*-a+*.state[2]}")])
    assert e.value.rc == EINVAL
    with pytest.raises(native.HtkAmdError, match="rather long for a macro name") as e:
        m.tie("X" * 21, "{*-a+*.state[2]}")
    assert e.value.rc == EINVAL
    with pytest.raises(native.HtkAmdError, match="bad cluster count") as e:
        m.data_cluster(None, [("NC", 0, "X_", "{*-a+*.state[2]}")])
    assert e.value.rc == EINVAL
    m.tie("S_b_2", "{*-b+*.state[2]}")                                # a state that is a ~s macro already: the tree path's wording
    with pytest.raises(native.HtkAmdError, match="is the ~s macro S_b_2 already: tying tied states is not supported") as e:
        m.data_cluster(None, [("TC", 1.0, "X_", "{*-b+*.state[2]}")])
    assert e.value.rc == EMODEL
    with pytest.raises(native.HtkAmdError, match="is the ~t macro T_a already") as e:
        m.tie("T_x", "{*-a+*.transP}")
    assert e.value.rc == EMODEL
    for items, reason in (("{*-a+*}", "whole models"), ("{*-a+*.state[2].mix[1]}", "items below the state"), ("{*-a+*.state[2],*-a+*.transP}", "different types")):
        with pytest.raises(native.HtkAmdError, match=reason) as e:
            m.tie("Y_", items)
        assert e.value.rc == EINVAL


HDR = "~o <STREAMINFO> 1 2 <VECSIZE> 2 <NULLD><USER>%s\n"
TRANS = "<TRANSP> 3\n0 1 0\n0 .5 .5\n0 0 0\n<ENDHMM>\n"
VAR = "<VARIANCE> 2\n1 1\n"
ONE = "<MEAN> 2\n0 0\n" + VAR


def hmm(name, body):
    return '~h "%s"\n<BEGINHMM>\n<NUMSTATES> 3\n<STATE> 2\n%s%s' % (name, body, TRANS)


def test_sets_outside_the_path_are_refused(native, tmp_path):
    sets = {
        "fullc": (HDR % "<FULLC>" + hmm("a", "<MEAN> 2\n0 0\n<INVCOVAR> 2\n2 0.5\n1\n"), "FULLC sets are not supported"),
        "streams": ("~o <STREAMINFO> 2 1 1 <VECSIZE> 2 <NULLD><USER><DIAGC>\n" +
                    hmm("a", "<STREAM> 1\n<MEAN> 1\n0\n<VARIANCE> 1\n1\n<STREAM> 2\n<MEAN> 1\n0\n<VARIANCE> 1\n1\n"), "more than one stream"),
        "tiedmix": (HDR % "<DIAGC>" + '~m "TM_1_1"\n' + ONE + '~m "TM_1_2"\n<MEAN> 2\n1 1\n' + VAR + hmm("a", '<NUMMIXES> 2\n<TMIX> "TM_1_"\n 0.5 0.5\n'),
                    "tied-mixture sets are not supported"),
        "discrete": (HDR.replace("<USER>", "<DISCRETE>") % "<DIAGC>" + hmm("a", ONE), "discrete sets are not supported"),
    }
    for name, (text, reason) in sets.items():
        p = tmp_path / name
        p.write_text(text)
        m = native.Mmf(files=[str(p)])
        with pytest.raises(native.HtkAmdError, match=reason) as e:
            m.data_cluster(None, [("TC", 1.0, "X_", "{a.state[2]}")])
        assert e.value.rc == EMODEL, name


def test_an_empty_item_list_is_a_warning(native, fixture_set):
    if native.lib().htkamd_device_count() > 0:
        pytest.skip("a GPU is present")
    assert fixture_set.data_cluster(None, [("TC", 1.0, "X_", "{z-z+z.state[2]}")]) == [0]      # nothing left for the device: no error
    assert "no items to cluster for X_" in fixture_set.last_warning


def test_ti_gives_hhed_s_file_byte_for_byte(native, tmp_path):
    from htk_amd import treeclust
    m = load_sub(native, tmp_path, "sub_untied.mmf")
    sc = treeclust.parse_script(open(os.path.join(du.G, "d.hed")).read())
    assert [c[0] for c in sc.commands] == ["TI", "TI"]
    treeclust.run_script(m, sc)
    out = tmp_path / "tied.mmf"
    m.write(m.packed(), one_file=str(out))
    assert out.read_bytes() == du.golden_bytes("tied_d.mmf")
    pk = m.packed()
    assert len(set(pk["hmmTrans"].tolist())) == 1                     # one matrix for all twenty models


def test_no_device_errors(native, fixture_set):
    if native.lib().htkamd_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(native.HtkAmdError, match="no HIP device") as e:
        fixture_set.data_cluster(None, [("TC", 1.0, "X_", "{*-a+*.state[2]}")])
    assert e.value.rc == ENODEV
    with pytest.raises(native.HtkAmdError, match="no HIP device"):
        native.state_distances(fixture_set, "{*-a+*.state[2]}")
    with pytest.raises(native.HtkAmdError, match="no HIP device"):
        native.cluster_merges(np.ones((3, 3), np.float32))


def test_symbols_are_present(native):
    L = native.lib()
    for name in ("htkamd_mmf_data_cluster", "htkamd_mmf_tie", "htkamd_state_distances", "htkamd_cluster_merges"):
        assert hasattr(L, name), name
    hdr = open(os.path.join(tu.ROOT, "include", "htk_amd.h")).read()
    assert "htkamd_cluster_spec" in hdr and "the reference only warns" in hdr
