"""The VQ table on the host (host/vqtab.c) against the files the reference's HQuant wrote (tests/golden/vq, make_vq_golden.py), the
DISCRETE writer against the reference's HCopy, and every refusal of the VQ calls that needs no device."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vq")
TABLES = ["lin", "lin_g", "tree"]


def read(path):
    return open(path, "rb").read()


@pytest.mark.parametrize("name", TABLES)
def test_read_write_round_trips_the_golden_table(native, name, tmp_path):
    tab = native.VQ(path=os.path.join(GOLD, name + ".vq"), magic=262)
    tab.write(str(tmp_path / "t.vq"))
    assert read(tmp_path / "t.vq") == read(os.path.join(GOLD, name + ".vq"))
    assert (tab.type, tab.kind) == ((native.VQ_BINTREE, native.CK_FULLC) if name == "tree" else (native.VQ_LINTREE, native.CK_INVDIAGC))


@pytest.mark.parametrize("name", TABLES)
def test_node_numbering_from_cluster_sets(native, name, tmp_path):
    """AddLinEntries (the list starts at the last cluster) and AddBinEntries (leaves are the nodes above numClust / 2): the golden
    table's nodes put back into cluster order, made into a table again, give the golden bytes."""
    tab = native.VQ(path=os.path.join(GOLD, name + ".vq"))
    sets = []
    for s in range(tab.num_streams):
        st = tab.stream(s)
        n = len(st["vqidx"])
        if tab.type == native.VQ_LINTREE:
            assert list(st["vqidx"]) == list(range(n, 0, -1))
            order = np.argsort(st["vqidx"])
        else:                                   # heap numbers from the walk: the root is 1, the children of h are 2h and 2h + 1
            heap = np.zeros(n, np.int64)
            heap[0] = 1
            for p in range(n):
                if st["left"][p] >= 0:
                    heap[st["left"][p]], heap[st["right"][p]] = 2 * heap[p], 2 * heap[p] + 1
            order = np.argsort(heap)
            leaves = heap > n // 2
            assert np.array_equal(st["vqidx"][leaves], heap[leaves] - n // 2) and not st["vqidx"][~leaves].any()
        sets.append(dict(size=np.ones(n, np.int32), centre=st["mean"][order], cov=st["cov"][order], tree=tab.type == native.VQ_BINTREE))
    native.VQ(clusters=sets, kind=tab.kind, magic=tab.magic).write(str(tmp_path / "t.vq"))
    assert read(tmp_path / "t.vq") == read(os.path.join(GOLD, name + ".vq"))


def test_gconst_is_create_vq_nodes(native):
    st = native.VQ(path=os.path.join(GOLD, "lin.vq")).stream(0)
    for g, iv in zip(st["gconst"], st["cov"]):
        s = np.float32(6 * np.log(6.28318530717959))
        for v in iv:
            s = np.float32(np.float64(s) - np.log(np.float64(v)))
        assert g == s


def test_discrete_file_is_hcopys(native, tmp_path):
    gold = read(os.path.join(GOLD, "tree_a.dis"))
    codes = np.frombuffer(gold[12:-2], ">i2").reshape(-1, 2)      # (HCopy adds the check sum: SAVEWITHCRC is on by default)
    native.parm_write_discrete(str(tmp_path / "a.dis"), codes, 100000, withCrc=True)
    assert read(tmp_path / "a.dis") == gold


REFUSED_TABLES = [
    ("1 0 0 1 1 2 \n1 1 1 0 0\n 0 0\n", 6172, "DIAGC"), ("1 0 5 2 1 2 \n1 1 1 0 3\n 0 0\n\n1 2 2 0 0\n 1 1\n\n", -6, "cannot find node 3"),
    ("1 2 5 1 1 2 \n", -6, "tree type"), ("1 0 5 1 1 2 \n1 1 1 0 0\n 0\n", -6, "mean vector"), ("7 0 5 1 1 2 \n1 1 1 0 0\n 0 0\n", -1, "magic=7")]


@pytest.mark.parametrize("text, rc, word", REFUSED_TABLES)
def test_table_files_refused(native, text, rc, word, tmp_path):
    (tmp_path / "bad.vq").write_text(text)
    with pytest.raises(native.HtkAmdError, match=word) as e:
        native.VQ(path=str(tmp_path / "bad.vq"), magic=1)
    assert e.value.rc == rc


@pytest.mark.parametrize("args, rc, word", [
    (dict(N=4, D=3, nc=5), 7120, "only 4 items"), (dict(N=64, D=3, nc=6, tree=True), 7172, "power of 2"), (dict(N=64, D=129, nc=2), -1, "maximum is 128"),
    (dict(N=2000, D=3, nc=1025), -1, "maximum is 1024"), (dict(N=64, D=3, nc=2, dist_kind=3), 7170, "cov kind"),
    (dict(N=64, D=3, nc=2, dist_kind=1), -1, "needs its covariance")])
def test_cluster_calls_refused_before_a_device_is_touched(native, args, rc, word):
    with pytest.raises(native.HtkAmdError, match=word) as e:
        native.vq_cluster(8, **args)                  # (the address is never read)
    assert e.value.rc == rc


def test_coder_and_table_refusals(native):
    tab = native.VQ(path=os.path.join(GOLD, "tree.vq"))
    with pytest.raises(native.HtkAmdError, match="add up to 6, the data has 5 columns"):
        tab.code(8, [0, 4], 5)
    one = dict(size=np.ones(1, np.int32), centre=np.zeros((1, 2), np.float32), cov=np.ones((1, 2), np.float32))
    with pytest.raises(native.HtkAmdError, match="DIAGC") as e:
        native.VQ(clusters=[one], kind=native.CK_DIAGC)
    assert e.value.rc == 6172
    bad = dict(one, cov=np.array([[1, 2, 1]], np.float32))
    with pytest.raises(native.HtkAmdError, match="not invertible") as e:
        native.VQ(clusters=[bad], kind=native.CK_FULLC)
    assert e.value.rc == 5220


@pytest.mark.parametrize("sw, ok", [("-d", True), ("-f", True), ("-g", True), ("-n", True), ("-s", True), ("-t", True), ("-F", True),
                                    ("-G", False), ("-H", False), ("-I", False), ("-L", False), ("-X", False), ("-l", False), ("-w", False), ("-q", False)])
def test_hquant_switches(native, sw, ok):
    if ok:
        native.hquant_check_switch(sw)
    else:
        with pytest.raises(native.HtkAmdError, match=sw):
            native.hquant_check_switch(sw)
