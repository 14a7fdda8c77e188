"""HLStats' and HBuild's host side without a device: the probabilities and the writers from PLANTED integer counts against the reference's
files (tests/golden/lm, made by tests/golden/make_lm_golden.py), the model reader, the refusals, the word loop.  The arcs of the -n and -m
networks are written by a kernel: those networks are compared with HBuild's SLF in tests/test_gpu_lstats.py, not here."""
import os
import subprocess

import numpy as np
import pytest

from htk_amd import capi
import lm_cases as lc

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "_ref")


def planted(case, spec):
    d, words, utts, _ = lc.load_case(case)
    enter, exit_ = lc.boundary(spec)
    ls = capi.LabelStats(words, enter, exit_)
    ids, times = lc.case_ids(ls, utts)
    V = ls.n + 1
    count, pairs, durs = lc.gather(ids, V, ls.id(enter), ls.id(exit_), times)
    rowOff, succ, cnt = lc.csr(pairs, V)
    dsum = np.array([sum(durs.get(w, [])) for w in range(V)], np.int64)
    dmin = np.array([min(durs[w]) if w in durs else np.iinfo(np.int64).max for w in range(V)], np.int64)
    dmax = np.array([max(durs[w]) if w in durs else np.iinfo(np.int64).min for w in range(V)], np.int64)
    return ls.plant(len(utts), count, rowOff, succ, cnt, (dsum, dmin, dmax))


def test_word_order_is_the_references():
    ls = capi.LabelStats(["b", "zz", "a", "!EXIT"])
    assert ls.words == ["!NULL", "!ENTER", "a", "b", "zz", "!EXIT"]
    assert [ls.id(w) for w in ("!ENTER", "a", "zz", "!EXIT", "nope")] == [1, 2, 4, 5, 0]


@pytest.mark.parametrize("case,name", [(c, v) for c, v in lc.variants() if lc.load_case(c)[3][v]["hlstats"] is not None])
def test_files_from_planted_counts(case, name, tmp_path):
    d, _, _, manifest = lc.load_case(case)
    got = lc.run_variant(capi, planted(case, manifest[name]), manifest[name], str(tmp_path), name)
    for suffix, data in got.items():
        assert data == open(os.path.join(d, name + "." + suffix), "rb").read(), suffix


def test_unknown_label_goes_to_the_null_slot():
    """GatherStats gives a label outside the list id 0: it is counted in the predecessor's total but is nobody's successor or predecessor."""
    d, words, utts, manifest = lc.load_case("toy")
    ls = planted("toy", manifest["bo"])
    t = ls.tables()
    b = ls.id("b")
    row = dict(zip(t["succ"][t["rowOff"][b]:t["rowOff"][b + 1]], t["cnt"][t["rowOff"][b]:t["rowOff"][b + 1]]))
    assert row[0] == 1 and t["count"][0] == 1


@pytest.mark.parametrize("case,name", [(c, v) for c, v in lc.variants() if lc.load_case(c)[3][v]["hbuild"] is not None and lc.load_case(c)[3][v]["hlstats"] is not None])
def test_model_reader(case, name):
    """What the reader keeps is what the file says: the text of every number read back to the file's four decimals."""
    d, _, _, _ = lc.load_case(case)
    lm = capi.Bigram(os.path.join(d, name + ".bigram"))
    text = open(os.path.join(d, name + ".bigram")).read()
    t = lm.tables()
    if lm.type == capi.LM_MATRIX:
        rows = [l.split() for l in text.splitlines()]
        assert [r[0] for r in rows] == lm.words[1:]
        for i, r in enumerate(rows, 1):
            vals = []
            for tok in r[1:]:
                x, _, rep = tok.partition("*")
                vals += [np.float32(x)] * int(rep or 1)
            want = np.array([np.float32(-1.0e10) if float(v) < 2.45e-308 else np.float32(np.log(np.float64(v))) for v in vals], np.float32)
            assert np.array_equal(t["mat"][i, 1:], want)
    else:
        uni = text.split("\\1-grams:\n")[1].split("\n\n")[0].splitlines()
        assert [l.split("\t")[1] for l in uni] == lm.words[1:]
        assert np.array_equal(t["unigram"][1:], np.array([np.float32(float(np.float32(l.split("\t")[0])) * 2.30258509299404568) for l in uni], np.float32))
        assert list(t["hasEntry"][1:]) == [int(len(l.split("\t")) == 3) for l in uni]
        big = text.split("\\2-grams:\n")[1].split("\n\n")[0].splitlines()
        assert len(big) == len(t["succ"]) == t["rowOff"][-1]
        pairs = [(lm.words.index(l.split("\t")[1].split()[0]), lm.words.index(l.split("\t")[1].split()[1])) for l in big]
        got = [(i, int(s)) for i in range(1, lm.n + 1) for s in t["succ"][t["rowOff"][i]:t["rowOff"][i + 1]]]
        assert got == pairs


def test_word_loop(tmp_path):
    d, words, _, manifest = lc.load_case("toy")
    for name in ("loop", "loop_t"):
        _, data = lc.build_net(capi, d, words, name, manifest[name], str(tmp_path))
        assert data == open(os.path.join(d, name + ".slf"), "rb").read()


@pytest.mark.parametrize("tool,sw", [("lstats", "-p"), ("lstats", "-h"), ("lstats", "-q"), ("netbuild", "-x"), ("netbuild", "-w"), ("netbuild", "-L"),
                                     ("netbuild", "-j"), ("netbuild", "-b")])
def test_refusals_name_the_switch(tool, sw):
    L = capi.lib()
    assert getattr(L, "htkamd_%s_check_switch" % tool)(sw.encode()) == -1
    assert sw in L.htkamd_last_error().decode()


def test_served_switches():
    L = capi.lib()
    assert all(L.htkamd_lstats_check_switch(("-" + c).encode()) == 0 for c in "botufscdlIGLX")
    assert all(L.htkamd_netbuild_check_switch(("-" + c).encode()) == 0 for c in "mnstuz")


def test_bad_calls_are_refused():
    ls = capi.LabelStats(["a"])
    with pytest.raises(capi.HtkAmdError, match="nothing has been counted"):
        ls.bigram_write("/dev/null")
    with pytest.raises(capi.HtkAmdError, match="both"):
        capi.LabelStats(["a"], "x", "x")
    with pytest.raises(capi.HtkAmdError, match="twice"):
        capi.LabelStats(["a", "a"])


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "HBuild")), reason="reference HBuild not built (make -C oracle _ref/HBuild)")
@pytest.mark.parametrize("name", ["bo", "mat_f001"])
def test_reference_hbuild_reads_our_bigram(name, tmp_path):
    d, words, _, manifest = lc.load_case("rand12")
    lc.run_variant(capi, planted("rand12", manifest[name]), manifest[name], str(tmp_path), name)
    wl = tmp_path / "wl"
    wl.write_text("".join(w + "\n" for w in words + ["!ENTER", "!EXIT"]))
    subprocess.run([os.path.join(REF, "HBuild")] + manifest[name]["hbuild"] + [str(tmp_path / (name + ".bigram")), str(wl), str(tmp_path / "ref.slf")], check=True)
    assert (tmp_path / "ref.slf").read_bytes() == open(os.path.join(d, name + ".slf"), "rb").read()
