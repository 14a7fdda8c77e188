"""The host side of the scorer, no device: names -> ids as HResults normalises them, the text writers fed with the numbers parsed back
from the reference's own output (tests/golden/results, make_results_golden.py), the reference lookup, and the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from results_util import GOLD, RUNS, corner_pairs, grid_align, norm_pairs, parse_output, strip_date  # noqa: E402

LIST = [l.strip() for l in open(os.path.join(GOLD, "list"))]


def handle(native, sw, with_list=True):
    """The scorer a run's switches describe."""
    eq = [(sw[k + 1], sw[k + 2]) for k, s in enumerate(sw) if s == "-e"]
    return native.Results(null_name=sw[sw.index("-z") + 1] if "-z" in sw else None, equiv=eq, ignore_case="-c" in sw, strip="-s" in sw, nist="-n" in sw,
                          label_list=LIST if with_list else [])


def pairs_of(hyp):
    if hyp[0].endswith(".mlf"):
        return corner_pairs() if hyp[0].startswith("corner") else norm_pairs()
    out = []
    for p in hyp:
        lab = os.path.join(GOLD, "files", "lab", os.path.basename(p)[:-4] + ".lab")
        out.append((p, [l.split()[2] for l in open(lab)], [l.split()[2] for l in open(os.path.join(GOLD, p))]))
    return out


@pytest.mark.parametrize("run", sorted(RUNS))
def test_writer_reproduces_the_fixture_from_its_numbers(native, run, tmp_path):
    """H D S I N per file, the alignments and the confusion counts are read back from the fixture's text (what the text does not show
    -- the counts of a file without -f -- from the restated grid) and htkamd_results_write prints them again: the same bytes."""
    sw, hyp = RUNS[run]
    text = open(os.path.join(GOLD, run + ".out")).read()
    res = handle(native, sw)
    p = parse_output(text, res.label_id)
    pairs = pairs_of(hyp)
    mlf = hyp[0].endswith(".mlf")
    rec_files = [n + ".rec" for n, _, _ in pairs] if mlf else list(hyp)
    lab_files = [n + ".lab" for n, _, _ in pairs] if mlf else ["files/lab/" + os.path.basename(f)[:-4] + ".lab" for f in hyp]
    counts, aln, off = [], [], [0]
    shown = dict(p["files"])
    for (name, ref, test), rec, lab in zip(pairs, rec_files, lab_files):
        cell, triples = grid_align([res.label_id(w) for w in ref], [res.label_id(w) for w in test], "-n" in sw)
        c = [cell["hit"], cell["del"], cell["sub"], cell["ins"], cell["hit"] + cell["del"] + cell["sub"], 1]
        if "-f" in sw:
            assert shown[os.path.basename(rec)] == c[:5], (run, name)         # the restated grid against the reference, pair by pair
            c = shown[os.path.basename(rec)] + [1]
        if "-t" in sw:
            assert (lab in p["aligned"]) == bool(c[1] or c[2] or c[3]), (run, name)
            if lab in p["aligned"]:
                assert p["aligned"][lab] == (rec, triples), (run, name)
                triples = p["aligned"][lab][1]
        counts.append(c); aln += triples; off.append(len(aln))
    assert np.sum(np.array(counts)[:, :5], axis=0).tolist() == p["totals"][:5]
    conf = None
    if "-p" in sw:
        V = len(LIST)
        conf = np.zeros((V + 1, V + 1), np.int32)
        for (r, t), n in p["conf"].items():
            conf[0 if r == "Ins" else LIST.index(r) + 1, 0 if t == "Del" else LIST.index(t) + 1] = n
        mine = np.zeros_like(conf)
        for op, r, t in aln:
            mine[max(r, 0), max(t, 0)] += 1
        assert np.array_equal(mine, conf), run
    flags = (native.RES_FULL if "-f" in sw else 0) | (native.RES_TRANS if "-t" in sw else 0) | (native.RES_PSTATS if "-p" in sw else 0)
    out = str(tmp_path / "out.txt")
    res.write(flags, p["ref"], p["rec"], rec_files, lab_files, counts, p["totals"], aln_off=off, aln=np.array(aln + [(0, 0, 0)], np.int32), conf=conf, path=out)
    assert strip_date(open(out).read()) == strip_date(text)


def test_names_to_ids(native):
    """-s strips first, then -e (the last one given first), then -c; the null class is id 0; the list's names are ids 1..n."""
    r = native.Results(label_list=["a", "b"])
    assert [r.label_id(w) for w in ("a", "b", "???", "c", "a", "c", "l-a+r")] == [1, 2, 0, 3, 1, 3, 4]
    assert r.label_name(0) == "???" and r.label_name(3) == "c" and r.num_labels() == 5
    r = native.Results(strip=True, null_name="sil")
    assert r.label_id("l-a+r") == r.label_id("a") == r.label_id("x-a") == r.label_id("a+y") and r.label_id("l-sil+r") == 0
    assert r.label_name(r.label_id("a-b-c+d+e")) == "b-c+d"                     # behind the FIRST '-', before the LAST '+'
    r = native.Results(ignore_case=True, null_name="sil")
    assert r.label_id("Alpha") == r.label_id("ALPHA") == r.label_id("alpha") and r.label_name(r.label_id("alpha")) == "ALPHA"
    assert r.label_id("sil") != 0 and r.label_id("SIL") == r.label_id("sil")    # upper-cased, it is no longer the null class's name
    r = native.Results(equiv=[("a", "x"), ("b", "a")])
    assert r.label_id("a") == r.label_id("b") and r.label_name(r.label_id("x")) == "a"   # ("b", "a") is applied first, then ("a", "x"): x -> a, not b ...
    r = native.Results(equiv=[("b", "a"), ("a", "x")])
    assert r.label_name(r.label_id("x")) == "b" and r.label_name(r.label_id("a")) == "b"    # ... and the other way round x -> a -> b
    r = native.Results(equiv=[("a", "x")], strip=True, ignore_case=True)
    assert r.label_name(r.label_id("l-x+r")) == "A" and r.label_name(r.label_id("X")) == "X"


def test_fixture_names_imply_the_same_ids(native):
    """The -e, -c and -s runs print the normalised names: every printed name is what label_id makes of some raw label of the set."""
    for run in ("e", "c", "s", "z"):
        sw, hyp = RUNS[run]
        res = handle(native, sw, with_list=False)
        p = parse_output(open(os.path.join(GOLD, run + ".out")).read(), res.label_id)
        raw = set(w for _, ref, test in pairs_of(hyp) for w in ref + test)
        made = set(res.label_name(res.label_id(w)) for w in raw)
        printed = set(res.label_name(i) for _, tr in p["aligned"].values() for _, r, t in tr for i in (r, t) if i >= 0)
        assert printed and printed <= made, run
        if run == "z":
            assert "sil" not in printed and res.label_id("sil") == 0


def test_reference_lookup(native, tmp_path):
    res = native.Results()
    mlf = native.Mlf(os.path.join(GOLD, "corner.ref.mlf"))
    i, lab = res.ref_for("some/dir/tie_short.rec", [mlf])
    assert lab == "some/dir/tie_short.lab" and res.label_name(1) == "a"
    assert res.ref_for("tie_short.rec", [mlf], lab_dir="some/dir") == (i, lab)               # the same reference, once
    j, lab = res.ref_for("tie_long.rec", [mlf])
    assert j == i + 1 and lab == "tie_long.lab"
    k, lab = res.ref_for("x/u1.rec", [mlf], lab_dir=os.path.join(GOLD, "files", "lab"))      # not in the MLF: the file
    assert lab == os.path.join(GOLD, "files", "lab", "u1.lab")
    k, lab = res.ref_for("u2.rec", [], lab_dir=os.path.join(GOLD, "files", "rec"), lab_ext="rec")
    assert lab.endswith("files/rec/u2.rec")
    with pytest.raises(native.HtkAmdError, match=r"no reference transcription for nowhere/zz\.rec: nowhere/zz\.lab"):
        res.ref_for("nowhere/zz.rec", [mlf])


@pytest.mark.parametrize("sw,word", [("-w", "word spotting"), ("-u", "word spotting"), ("-k", "per-speaker"), ("-h", "NIST output format"), ("-d", "N-best"),
                                     ("-m", "limit"), ("-j", "limit"), ("-a", "phrase label"), ("-b", "phone label")])
def test_out_of_scope_switches_are_refused_by_name(native, sw, word):
    with pytest.raises(native.HtkAmdError, match=r"switch %s \(.*%s.*\) is not supported" % (sw, word)):
        native.results_check_switch(sw)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import hresults_score
    with pytest.raises(native.HtkAmdError, match="switch %s " % sw):
        hresults_score.main([sw, "1", os.path.join(GOLD, "list"), os.path.join(GOLD, "corner.rec.mlf")])


def test_other_refusals(native):
    for sw in "ecsznftpILX":
        native.results_check_switch("-" + sw)
    with pytest.raises(native.HtkAmdError, match="unknown switch -q"):
        native.results_check_switch("-q")
    with pytest.raises(native.HtkAmdError, match="label level 2 is not supported"):
        native.Results(ref_level=2)
    with pytest.raises(native.HtkAmdError, match="label level 1 is not supported"):
        native.Results(test_level=1)
    res = native.Results(label_list=["a"])
    i = res.add_ref("u", ["a", "b"])
    with pytest.raises(native.HtkAmdError, match="label b is not in the list"):          # Index HResults.c:1151
        res.score([i], [[res.ids_of(["a"])]], conf=True)
    with pytest.raises(native.HtkAmdError, match="names reference 7 of 1"):
        res.score([7], [[res.ids_of(["a"])]])
