"""tests/regtree_ref.py, the float32 restatement the regression class tree's kernels are compared with (tests/test_gpu_regtree_kernels.py),
is itself pinned to HHEd here, without a GPU: over the member arrays recorded beside the nine cases (steps.npz, written by
tests/golden/make_regtree_golden.py) it must make the recorded device steps -- the same ranges, the same seeds bit for bit -- and end in the
class lists of HHEd's rtree.base, the tree of HHEd's rtree.tree and the per-split CalcDistance counts of HHEd's trace."""
import json
import os

import numpy as np
import pytest

import regtree_ref as rr
import regtree_util as ru


def load_case(name):
    """(RegTreeRef over the case's members, the recorded steps as capi.regtree_probe takes them, the npz)."""
    z = np.load(os.path.join(ru.GOLDEN, name, "steps.npz"))
    ref = rr.RegTreeRef(z["mean"], z["sum"], z["sqr"], z["occ"], z["has"])
    steps = [("split", int(o), int(n), s) if k else ("node", int(o), int(n)) for k, o, n, s in zip(z["step_split"], z["step_off"], z["step_n"], z["step_seeds"])]
    return ref, steps, z


@pytest.mark.parametrize("name", sorted(ru.CASES))
def test_restatement_reproduces_hhed(name):
    d = os.path.join(ru.GOLDEN, name)
    ref, recorded, z = load_case(name)
    assert int(z["n_terminals"]) == ru.CASES[name][1] and ref.D == ru.CASES[name][0]["D"]
    steps, results, kids, ranges = rr.build_tree(ref, int(z["n_terminals"]), int(z["n_nonspeech"]))
    # the steps the restatement makes are the recorded ones
    assert [s[:3] for s in steps] == [s[:3] for s in recorded]
    for s, r in zip(steps, recorded):
        if s[0] == "split":
            assert np.array_equal(np.asarray(s[3], np.float32).view(np.uint32), r[3].view(np.uint32))
    # and stepping over the recorded ones gives the same figures and the same list
    again, steps2, _ = load_case(name)
    results2, list2 = rr.run_steps(again, steps2)
    assert np.array_equal(list2, ref.list)
    for a, b in zip(results, results2):
        if isinstance(a, tuple):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        else:
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # HHEd's files and trace
    assert kids == ru.parse_tree(open(os.path.join(d, "rtree.tree")).read())
    members = list(zip(z["model"].tolist(), z["state"].tolist(), z["mix"].tolist()))
    classes = [[members[i] for i in list2[off:off + n]] for (left, _), (off, n) in zip(kids, ranges) if not left]
    assert classes == ru.parse_base(open(os.path.join(d, "rtree.base")).read())
    assert [int(r[0][2]) for r in results2 if isinstance(r, tuple)] == json.load(open(os.path.join(ru.GOLDEN, "iterations.json")))[name]
    for r in results2:
        if isinstance(r, tuple):
            assert int(r[0][0]) + int(r[0][1]) > 0 and sorted(list2.tolist()) == list(range(ref.G))


def test_chain_is_sequential_from_plus_zero():
    """The sums of the restatement: one float32 add after another in row order (not pairwise), and an all-minus-zero column sums to +0."""
    rng = np.random.RandomState(3)
    rows = (rng.randn(300, 2) * np.exp(3 * rng.randn(300, 2))).astype(np.float32)
    want = np.zeros(2, np.float32)
    for r in rows:
        want = want + r
    assert np.array_equal(rr.chain(rows).view(np.uint32), want.view(np.uint32))
    assert rr.chain(rows)[0] != np.float32(rows[:, 0].astype(np.float64).sum())      # the inputs make the order show
    assert not np.signbit(rr.chain(np.full((3, 1), -0.0, np.float32)))[0]
    assert np.array_equal(rr.chain(np.zeros((0, 4), np.float32)), np.zeros(4, np.float32))
