"""htkamd_results_score on the device against the reference's HResults: the committed runs of tests/golden/make_results_golden.py byte
for byte (all but the Date: line), the corner pairs' counts and alignment triples against a plain restatement of the reference's grid,
several hypothesis sets in one call, a randomised sweep against oracle/_ref/HResults itself, and the demo's published result blocks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from results_util import GOLD, RUNS, corner_pairs, grid_align, strip_date  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "golden", "demo")
HRESULTS = os.path.join(ROOT, "oracle", "_ref", "HResults")
sys.path.insert(0, os.path.join(ROOT, "examples"))


def run_script(argv, out):
    import hresults_score
    hresults_score.main(argv)
    return open(out).read()


@pytest.mark.parametrize("run", sorted(RUNS))
def test_fixture_run_through_the_script(native, run, tmp_path, monkeypatch):
    """examples/hresults_score.py with the run's switches, inside the fixture directory: the reference's standard output."""
    monkeypatch.chdir(GOLD)
    sw, hyp = RUNS[run]
    out = str(tmp_path / "out.txt")
    got = run_script(["--out", out] + sw + ["list"] + hyp, out)
    assert strip_date(got) == strip_date(open(os.path.join(GOLD, run + ".out")).read())


def score_pairs(native, pairs, nist, null_name="sil"):
    res = native.Results(null_name=null_name, nist=nist)
    refs = [res.add_ref(name, ref) for name, ref, _ in pairs]
    hyps = [res.ids_of(hyp) for _, _, hyp in pairs]
    return res, res.score(refs, [hyps], align=True)


@pytest.mark.parametrize("nist", [False, True])
def test_corner_pairs_counts_and_triples(native, nist):
    """Every corner pair, "sil" the null class, plus the pairs HResults cannot read (an empty side: the grid's edge cells, status 0):
    H D S I N and the triples equal the restated grid's, under both rule sets.  The pair `long` runs the global-scratch `dir` path,
    the others the LDS tile; r130_one and w65 take more than one 64-column stripe."""
    pairs = corner_pairs() + [("e_r", [], ["a", "sil", "b"]), ("e_t", ["a", "sil", "b"], []), ("e_both", [], [])]
    tile = native.lib().htkamd_results_dir_tile()
    assert [n for n, r, t in pairs if len(r) * len(t) > tile] == ["long"]
    res, got = score_pairs(native, pairs, nist)
    for u, (name, ref, hyp) in enumerate(pairs):
        rid, tid = [res.label_id(w) for w in ref], [res.label_id(w) for w in hyp]
        cell, triples = grid_align(rid, tid, nist)
        want = [cell["hit"], cell["del"], cell["sub"], cell["ins"], cell["hit"] + cell["del"] + cell["sub"], int(bool(ref) and bool(hyp))]
        assert got["counts"][0, u].tolist() == want, (name, nist)
        assert got["aln"][0][u].tolist() == [list(t) for t in triples], (name, nist)
        ops = got["aln"][0][u][:, 0].tolist()
        assert [ops.count(k) for k in (native.RES_HIT, native.RES_DEL, native.RES_SUB, native.RES_INS)] == want[:4], name
    counted = [u for u, p in enumerate(pairs) if p[1] and p[2]]
    assert got["totals"][0, :5].tolist() == got["counts"][0, counted, :5].sum(axis=0).tolist()
    assert got["totals"][0, 5] == len(counted)
    assert got["totals"][0, 6] == sum(1 for u in counted if not got["counts"][0, u, 1:4].any())


def test_three_sets_in_one_call_equal_three_calls(native):
    rng = np.random.default_rng(5)
    words = list("abcde") + ["sil"]
    refs = [[words[k] for k in rng.integers(0, 6, rng.integers(1, 50))] for _ in range(37)]
    sets = [[[words[k] for k in rng.integers(0, 6, rng.integers(1, 50))] for _ in refs] for _ in range(3)]
    res = native.Results(null_name="sil", label_list=words)
    ri = [res.add_ref("u%d" % u, r) for u, r in enumerate(refs)]
    ids = [[res.ids_of(h) for h in s] for s in sets]
    one = res.score(ri, ids, align=True, conf=True)
    for k in range(3):
        alone = res.score(ri, [ids[k]], align=True, conf=True)
        assert np.array_equal(one["counts"][k], alone["counts"][0])
        assert np.array_equal(one["totals"][k], alone["totals"][0])
        assert np.array_equal(one["conf"][k], alone["conf"][0])
        for u in range(len(refs)):
            assert np.array_equal(one["aln"][k][u], alone["aln"][0][u])
    assert one["conf"][:, 1:, 1:].sum() + one["conf"][:, 1:, 0].sum() == one["totals"][:, 4].sum()     # every reference label is in a row
    assert one["conf"][:, 0, 1:].sum() == one["totals"][:, 3].sum()


@pytest.mark.parametrize("nist", [False, True])
def test_random_sweep_against_hresults(native, nist, tmp_path):
    """300 pairs of lengths 1-40 (HResults cannot read an empty transcription), five words and a null class: the script's -f -t -p text
    is oracle/_ref/HResults's, so every pair's counts, every alignment with an error and the confusion matrix are compared."""
    if not os.path.exists(HRESULTS):
        pytest.skip("oracle/_ref/HResults is not built (no reference tree on this machine)")
    rng = np.random.default_rng(11 + nist)
    words = list("abcde") + ["sil"]
    (tmp_path / "list").write_text("".join(w + "\n" for w in words))
    with open(tmp_path / "ref.mlf", "w") as fr, open(tmp_path / "rec.mlf", "w") as ft:
        fr.write("#!MLF!#\n"); ft.write("#!MLF!#\n")
        for u in range(300):
            ref = [words[k] for k in rng.integers(0, 6, rng.integers(1, 41))]
            if u % 3 == 0:                                       # a third of the hypotheses are edits of the reference, the rest unrelated
                hyp = [w for w in ref if rng.random() > 0.15] or ["a"]
            else:
                hyp = [words[k] for k in rng.integers(0, 6, rng.integers(1, 41))]
            fr.write('"*/p%03d.lab"\n%s.\n' % (u, "".join(w + "\n" for w in ref)))
            ft.write('"*/p%03d.rec"\n%s.\n' % (u, "".join(w + "\n" for w in hyp)))
    sw = (["-n"] if nist else []) + ["-z", "sil", "-f", "-t", "-p", "-I", "ref.mlf", "list", "rec.mlf"]
    want = subprocess.run([HRESULTS] + sw, cwd=tmp_path, stdout=subprocess.PIPE, text=True, check=True).stdout
    import hresults_score
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        hresults_score.main(["--out", "got.txt"] + sw)
    finally:
        os.chdir(cwd)
    got = (tmp_path / "got.txt").read_text()
    assert sum(l.startswith("p") and ".rec:" in l for l in want.splitlines()) == 300
    assert strip_date(got) == strip_date(want)


def test_demo_rec_files_give_the_published_results(native, tmp_path):
    """The demo's recognition step on the device (as tests/test_gpu_demo.py runs it), its .rec files scored as runDemo does
    (HResults -s -L labels bcplist *.rec): the SENT: and WORD: lines of HTKDemo/results/monPlainM1S1.res for both sets."""
    from decode_util import format_words
    import hresults_score
    res_lines = open(os.path.join(DEMO, "monPlainM1S1.res")).read().splitlines()
    published = {"train": res_lines[res_lines.index("Training Set"):res_lines.index("Test Set")], "test": res_lines[res_lines.index("Test Set"):]}
    mmf = native.Mmf(hmm_list=os.path.join(DEMO, "bcplist"), hmm_dir=os.path.join(DEMO, "hmm_final"))
    model = native.Model(mmf.packed())
    net = native.Net(os.path.join(DEMO, "monLattice"), os.path.join(DEMO, "bcpvocab"), mmf)
    dec = native.Decoder(model, net, lmScale=0.0)
    expected = json.load(open(os.path.join(DEMO, "hvite_expected.json")))
    for part, labdir in (("test", "labels_test"), ("train", "labels")):
        names = sorted(expected[part])
        stat = [native.parm_read(os.path.join(DEMO, part, u + ".mfc"))[0] for u in names]
        dX, frameOff, cols = native.parm_add_qualifiers(stat, hasD=True)
        feats = dX.to_host(np.float32, (int(frameOff[-1]), cols))
        out = dec.run([feats[frameOff[u]:frameOff[u + 1]] for u in range(len(names))], genBeam=300.0, lmScale=0.0, wordPen=5.0)
        recs = []
        for u, (words, total) in zip(names, out):
            recs.append(str(tmp_path / (u + ".rec")))
            open(recs[-1], "w").write("".join(l + "\n" for l in format_words(words, net.out_syms)))
        txt = str(tmp_path / (part + ".res"))
        hresults_score.main(["--out", txt, "-s", "-L", os.path.join(DEMO, labdir), os.path.join(DEMO, "bcplist")] + recs)
        got = open(txt).read().splitlines()
        for key in ("SENT:", "WORD:"):
            assert [l for l in got if l.startswith(key)] == [l for l in published[part] if l.startswith(key)], part
