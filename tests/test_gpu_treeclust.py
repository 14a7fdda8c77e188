"""Decision-tree state clustering on the device (htk_amd/csrc/treeclust.hip + htk_amd/host/treeclust.c) against the reference's HHEd:
the split sums bit for bit against a sequential float32 restatement, the tied model set and the trees file byte for byte against the
committed HHEd outputs (tests/golden/make_treeclust_golden.py) and against HHEd run on the spot where its binary is there."""
import importlib.util
import json
import os

import numpy as np
import pytest

import treeclust_util as tu
from treeclust_util import G, ROOT

pytestmark = pytest.mark.gpu

HHED = os.path.join(ROOT, "oracle", "_ref", "HHEd")


def seq_sums(stats, items, answers):
    """[nQ][2][C]: every column added in list order, one float32 add at a time (np.add.accumulate over float32 is sequential)."""
    nQ, C = answers.shape[0], stats.shape[1]
    out = np.zeros((nQ, 2, C), np.float32)
    rows = stats[items]
    for q in range(nQ):
        a = answers[q, items].astype(bool)
        for side, sel in ((0, ~a), (1, a)):
            if sel.any():
                out[q, side] = np.add.accumulate(rows[sel], axis=0, dtype=np.float32)[-1]
    return out


@pytest.mark.parametrize("D", [1, 5, 39])
@pytest.mark.parametrize("nQ", [1, 64, 65])
def test_split_sums_are_bit_equal_to_sequential_float_adds(native, D, nQ):
    rng = np.random.RandomState(100 * D + nQ)
    nItems, C = 200, 2 * D + 1
    stats = (rng.randn(nItems, C) * np.exp(rng.randn(nItems, 1) * 3)).astype(np.float32)      # magnitudes apart: the order of the adds shows
    stats[:, 0] = np.abs(stats[:, 0])
    stats[rng.choice(nItems, 20, replace=False)] = 0.0                                         # states without occupation
    answers = (rng.rand(nQ, nItems) < 0.5).astype(np.uint8)
    answers[0] = 1                                                                             # an all-yes question
    if nQ > 1:
        answers[nQ - 1] = 0                                                                    # and an all-no one
    for n in (1, 2, 63, 64, 65, 130):
        items = rng.permutation(nItems)[:n].astype(np.int32)                                   # a shuffled subset: not table order
        got = native.tree_split_sums(stats, items, answers)
        want = seq_sums(stats, items, answers)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (D, nQ, n, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5])


def run_script(native, which, workdir, stats=None):
    from htk_amd import treeclust
    mmf_path, lst = tu.unpack_inputs(workdir)
    m = native.Mmf([mmf_path], hmm_list=lst)
    sc = treeclust.parse_script(open(os.path.join(G, "script%d.hed" % (3 if which == 3 else 1))).read())      # script 2 is script 1 without merging and leaf statistics
    warn = treeclust.run_script(m, sc, stats_path=stats or os.path.join(G, "stats"), merge=which != 2, leaf_stats=which != 2, base_dir=str(workdir))
    assert warn and "L_z" in warn                                     # the question no model answers is dropped, and said so
    m.write(m.packed(), one_file=os.path.join(str(workdir), "tied.mmf"))
    return m, open(os.path.join(str(workdir), "tied.mmf"), "rb").read(), open(os.path.join(str(workdir), sc.trees_path), "rb").read()


def first_difference(trees_got: bytes, which: int) -> str:
    """Where the trees part: the first split whose question is not the one HHEd's trace names (script 1), else the first differing line."""
    got = trees_got.decode().split("\n\n", 1)[1]
    if which == 1:
        for name, quests in json.load(open(os.path.join(G, "trace1.json")))["splits"]:
            blk = got.split(name + "\n", 1)[1].split("\n\n", 1)[0] if name + "\n" in got else ""
            mine = [ln.split()[1].strip("'") for ln in blk.splitlines() if ln.startswith(" ")]
            for k, qn in enumerate(quests):
                if k >= len(mine) or mine[k] != qn:
                    return "tree %s split %d: question %s, HHEd chose %s" % (name, k, mine[k] if k < len(mine) else None, qn)
    want = open(os.path.join(G, "trees%d" % which)).read().splitlines()
    for k, ln in enumerate(trees_got.decode().splitlines()):
        if k >= len(want) or ln != want[k]:
            return "trees line %d: %r, HHEd wrote %r" % (k + 1, ln, want[k] if k < len(want) else None)
    return "length"


@pytest.mark.parametrize("which", [1, 2, 3])
def test_scripts_give_hhed_s_files_byte_for_byte(native, tmp_path, which):
    _, mmf, trees = run_script(native, which, tmp_path)
    assert trees == open(os.path.join(G, "trees%d" % which), "rb").read(), first_difference(trees, which)
    assert mmf == tu.golden_bytes("tied%d.mmf" % which)


def test_live_against_hhed_with_other_occupations(native, tmp_path):
    if not os.path.exists(HHED):
        pytest.skip("oracle/_ref/HHEd is not built")
    spec = importlib.util.spec_from_file_location("make_treeclust_golden", os.path.join(ROOT, "tests", "golden", "make_treeclust_golden.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    (tmp_path / "ref").mkdir()
    mmf_path, lst = tu.unpack_inputs(tmp_path / "ref")
    base = native.Mmf([mmf_path], hmm_list=lst)
    gen.write_stats(base, str(tmp_path / "stats"), 23)
    assert open(tmp_path / "stats").read() != open(os.path.join(G, "stats")).read()
    (tmp_path / "ref" / "script1.hed").write_bytes(open(os.path.join(G, "script1.hed"), "rb").read())
    (tmp_path / "ref" / "stats").write_bytes(open(tmp_path / "stats", "rb").read())
    gen.run_hhed(str(tmp_path / "ref"), "hmmdefs", "hmmlist", "script1.hed", "tied.mmf")
    (tmp_path / "mine").mkdir()
    _, mmf, trees = run_script(native, 1, tmp_path / "mine", stats=str(tmp_path / "stats"))
    assert trees == open(tmp_path / "ref" / "trees", "rb").read()
    assert mmf == open(tmp_path / "ref" / "tied.mmf", "rb").read()


def test_the_tied_set_is_usable(native, tmp_path):
    m, _, trees = run_script(native, 1, tmp_path)
    pk = m.packed()
    leaves = set()
    for ln in trees.decode().splitlines():
        leaves.update(x.strip('"') for x in ln.split() if x.startswith('"ST_'))
    assert len(np.unique(pk["hmmState"])) == len(leaves) == pk["numStates"]
    m2 = native.Mmf([os.path.join(str(tmp_path), "tied.mmf")], hmm_list=os.path.join(str(tmp_path), "hmmlist"))      # the written file loads again
    pk2 = m2.packed()
    assert pk2["numStates"] == len(leaves)
    gm = native.Model(pk2)
    rng = np.random.RandomState(3)
    seqs = [np.array([m2.logical[n] for n in ("a-a+b", "c-a+d", "b-a+c")], np.int32), np.array([m2.logical[n] for n in ("e-a+e", "a-a+c")], np.int32)]
    feats = [rng.randn(40, pk2["vecSize"]).astype(np.float32), rng.randn(30, pk2["vecSize"]).astype(np.float32)]
    X = np.concatenate(feats)
    frameOff = np.array([0, 40, 70], np.int32); labOff = np.array([0, 3, 5], np.int32)
    dX = native.DevArray(X)
    fb, acc = native.ForwardBackward(gm), native.Accs(gm)
    fb.prepare(dX.ptr.value, frameOff, labOff, np.concatenate(seqs))
    fb.execute(native.fb_config(), acc)
    pr, st = fb.results()
    assert (st == 1).all() and np.isfinite(pr).all()
    a = acc.download()
    assert abs(a["muOcc"].sum() - 70.0) < 1e-2                        # every frame is somewhere
