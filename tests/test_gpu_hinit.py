"""HInit on the device (htk_amd/csrc/hinit.hip): FlatCluster for many pools in one launch bit for bit against the per-model example's
restatement, every model of the demo in one call against the reference's traces and model files (tests/golden/demo), one call against
one call per model, per-model statuses, the corners of tests/golden/hinit_set against the reference's HInit, and examples/hinit_set.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hinit_util as hu

pytestmark = pytest.mark.gpu

sys.path.insert(0, hu.ROOT)
NAMES = list("SCVNL")
HSET = os.path.join(hu.ROOT, "tests", "golden", "hinit_set")
HINIT = os.path.join(hu.ROOT, "oracle", "_ref", "HInit")


# ------------------------------------------------------------------------------------------ FlatCluster
@pytest.fixture(scope="module")
def cluster_case(native):
    """every pool of hinit_util.cluster_pools and one with fewer items than clusters; the pools of one vector size go into ONE launch
    (39 columns: 1, 4 and 16 clusters next to the pool that fails; 4 columns: the repair pool next to one that cannot be split), every
    launch is made twice; the restatement's answers"""
    pools = hu.cluster_pools()
    pools["one_cluster_39"] = (pools["dim_39"][0][:50] + np.float32(1.0), 1)
    pools["too_few"] = (np.arange(78, dtype=np.float32).reshape(2, 39), 3)
    by_dim = {}
    for name, (X, nc) in pools.items():
        by_dim.setdefault(X.shape[1], []).append(name)
    assert sorted(by_dim[39]) == ["dim_39", "many_39", "one_cluster_39", "too_few"] and sorted(by_dim[4]) == ["cannot_split", "repair"]
    first, second = {}, {}
    for D, names in by_dim.items():
        rows = np.concatenate([pools[n][0] for n in names])
        off = np.concatenate([[0], np.cumsum([pools[n][0].shape[0] for n in names])])
        lists = [np.arange(off[k], off[k + 1]) for k in range(len(names))]
        dX = native.DevArray(np.ascontiguousarray(rows))
        for out in (first, second):
            out.update(zip(names, native.flat_cluster(dX.ptr, rows.shape[0], D, lists, [pools[n][1] for n in names])))
    want = {}
    for name, (X, nc) in pools.items():
        try:
            want[name] = hu.flat_cluster_counted(X, nc)
        except ValueError:
            want[name] = None
    return pools, first, second, want


def same_bits(got, want, D):
    size, ctr, var, cmap, _ = want
    return (got["status"] == 0 and np.array_equal(got["size"], size) and np.array_equal(got["assign"], cmap) and
            np.array_equal(got["centre"][:, :D].view(np.uint32), ctr.view(np.uint32)) and np.array_equal(got["var"][:, :D].view(np.uint32), var.view(np.uint32)))


@pytest.mark.parametrize("name", ["one_cluster", "one_cluster_39", "three_per_cluster", "dim_1", "dim_39", "equidistant", "repair", "many_39"])
def test_flat_cluster_is_the_restatement_bit_for_bit(native, cluster_case, name):
    from examples.hinit_model import flat_cluster
    pools, first, _, want = cluster_case
    X, nc = pools[name]
    size, ctr, var = flat_cluster(X, nc)                                  # the counted copy IS the example's function
    assert np.array_equal(size, want[name][0]) and np.array_equal(ctr, want[name][1]) and np.array_equal(var, want[name][2])
    assert same_bits(first[name], want[name], X.shape[1]), name


def test_flat_cluster_pools_take_the_paths_they_are_there_for(cluster_case):
    pools, _, _, want = cluster_case
    assert pools["three_per_cluster"][0].shape[0] == 3 * pools["three_per_cluster"][1] and list(want["three_per_cluster"][0]) == [3, 3, 3, 3]
    assert want["repair"][4]["repairs"] >= 1                              # the restatement went through FullestCluster / Perturb again
    assert want["equidistant"][4]["ties"] >= 1                            # an item as far from one centre as from another: the first wins
    assert pools["dim_1"][0].shape[1] == 1 and pools["dim_39"][0].shape[1] == 39 and pools["one_cluster"][1] == 1
    assert want["cannot_split"] is None


def test_flat_cluster_failed_pools_have_a_status_and_leave_the_others_alone(native, cluster_case):
    _, first, _, _ = cluster_case
    assert first["too_few"]["status"] == native.HINIT_ECLUSTER and first["cannot_split"]["status"] == native.HINIT_ECLUSTER
    # (the other pools of the same launch are the ones test_flat_cluster_is_the_restatement_bit_for_bit compares)


def test_flat_cluster_twice_gives_the_same_bits(cluster_case):
    _, first, second, _ = cluster_case
    for name in first:
        assert first[name]["status"] == second[name]["status"]
        if first[name]["status"] == 0:
            for k in ("size", "assign", "centre", "var"):
                assert np.array_equal(first[name][k].view(np.uint32) if first[name][k].dtype == np.float32 else first[name][k],
                                      second[name][k].view(np.uint32) if second[name][k].dtype == np.float32 else second[name][k]), (name, k)


# ------------------------------------------------------------------------------------------ the demo
def demo_data(native, proto_dir):
    from examples.hinit_set import tokens_from_labels
    mmf = native.Mmf(hmm_list=os.path.join(hu.DEMO, "bcplist"), hmm_dir=proto_dir)
    files = sorted(f for f in os.listdir(os.path.join(hu.DEMO, "train")) if f.endswith(".mfc"))
    stat = [native.parm_read(os.path.join(hu.DEMO, "train", f))[0] for f in files]
    labels = [native.labels_read(os.path.join(hu.DEMO, "labels", f.replace(".mfc", ".lab"))) for f in files]
    dX, frame_off, cols = native.parm_add_qualifiers(stat, hasD=True)                     # TARGETKIND = MFCC_E_D over the whole file
    pk = mmf.packed()
    assert cols == pk["vecSize"]
    return mmf, pk, dX, frame_off, tokens_from_labels(pk, mmf.logical, frame_off, labels)


def run_demo(native, proto_dir, names=NAMES, tokens=None, **cfg):
    mmf, pk, dX, frame_off, tok = demo_data(native, proto_dir)
    tok = tok if tokens is None else tokens(mmf, tok)
    model, res = native.hinit(pk, dX.ptr, int(frame_off[-1]), tok, [mmf.logical[n] for n in names], native.hinit_config(max_iter=10, **cfg))
    return mmf, pk, model.get_params(), dict(zip(names, res))


@pytest.fixture(scope="module")
def demo_all(native):
    return run_demo(native, os.path.join(hu.DEMO, "proto"))


@pytest.fixture(scope="module")
def demo_mix_all(native):
    return run_demo(native, os.path.join(hu.DEMO, "hinit_mix", "proto"))


def check_against_reference(native, mmf, pk, p, res, name, log, ref_dir, weights=False):
    ref, converged = hu.ref_trace(log, name)
    r = res[name]
    assert r["status"] == native.HINIT_OK
    assert r["passes"] == len(ref) == len(r["logP"]), (name, r, ref)
    for x, rx in zip(r["logP"], ref):
        assert abs(x - rx) <= 1e-6 * abs(rx), (name, r["logP"], ref)
    assert r["converged"] == converged
    rmmf = native.Mmf(hmm_list=os.path.join(hu.DEMO, "bcplist"), hmm_dir=ref_dir)
    hu.compare_model(p, pk, mmf.logical[name], rmmf.packed(), rmmf.logical[name], weights=weights)


@pytest.mark.parametrize("name", NAMES)
def test_demo_all_models_in_one_call(native, demo_all, name):
    mmf, pk, p, res = demo_all
    check_against_reference(native, mmf, pk, p, res, name, os.path.join(hu.DEMO, "hinit_hrest.log"), os.path.join(hu.DEMO, "hmm0"))


@pytest.mark.parametrize("name", NAMES)
def test_demo_mixture_models_in_one_call(native, demo_mix_all, name):
    mmf, pk, p, res = demo_mix_all
    gold = os.path.join(hu.DEMO, "hinit_mix")
    check_against_reference(native, mmf, pk, p, res, name, os.path.join(gold, "hinit.log"), os.path.join(gold, "hmm0"), weights=True)
    h = mmf.logical[name]
    assert [int(pk["stateCompOff"][s + 1] - pk["stateCompOff"][s]) for s in pk["hmmState"][pk["hmmStateOff"][h]:pk["hmmStateOff"][h + 1]]] == [2, 3, 2]


@pytest.mark.parametrize("name", NAMES)
def test_one_call_over_five_models_equals_a_call_per_model(native, demo_all, name):
    mmf, pk, p, res = demo_all
    _, _, p1, res1 = run_demo(native, os.path.join(hu.DEMO, "proto"), names=[name])
    assert res1[name]["passes"] == res[name]["passes"] and res1[name]["converged"] == res[name]["converged"] and res1[name]["status"] == 0
    hu.compare_model(p, pk, mmf.logical[name], pk | p1, mmf.logical[name])
    # the call alone trained nothing else: the other models are the prototypes' bits
    proto = native.Model(pk).get_params()
    for other in NAMES:
        if other != name:
            assert hu.model_params_equal(p1, proto, pk, mmf.logical[other]), other


def test_a_model_with_too_few_tokens_keeps_its_prototype(native, demo_all):
    def two_of_v(mmf, tok):
        v = np.flatnonzero(tok[:, 2] == mmf.logical["V"])
        return np.delete(tok, v[2:], axis=0)
    mmf, pk, p, res = run_demo(native, os.path.join(hu.DEMO, "proto"), tokens=two_of_v, min_seg=3)
    assert res["V"]["status"] == native.HINIT_EFEWSEGS and res["V"]["passes"] == 0 and not res["V"]["converged"]
    assert hu.model_params_equal(p, native.Model(pk).get_params(), pk, mmf.logical["V"])
    for name in "SCNL":
        check_against_reference(native, mmf, pk, p, res, name, os.path.join(hu.DEMO, "hinit_hrest.log"), os.path.join(hu.DEMO, "hmm0"))


def test_a_model_whose_pools_cannot_be_clustered_is_put_back(native):
    """the restore inside a real call: V keeps two tokens of 3 frames, so each of its three pools has 2 items -- fewer than the 3 components
    of the middle state, and too few for two clusters of MIN_CLUST_SIZE 3 in the others.  k_hi_init raises the status and writes nothing;
    the call's end puts the model back from the snapshot and rebuilds its derived tables, beside four models that train as ever"""
    def two_short_of_v(mmf, tok):
        v = np.flatnonzero(tok[:, 2] == mmf.logical["V"])
        tok = np.delete(tok, v[2:], axis=0)
        tok[tok[:, 2] == mmf.logical["V"], 1] = 3
        return tok
    gold = os.path.join(hu.DEMO, "hinit_mix")
    mmf, pk, p, res = run_demo(native, os.path.join(gold, "proto"), tokens=two_short_of_v, min_seg=2)
    assert res["V"]["status"] == native.HINIT_ECLUSTER and res["V"]["passes"] == 0 and not res["V"]["converged"]
    assert hu.model_params_equal(p, native.Model(pk).get_params(), pk, mmf.logical["V"])
    for name in "SCNL":
        check_against_reference(native, mmf, pk, p, res, name, os.path.join(gold, "hinit.log"), os.path.join(gold, "hmm0"), weights=True)


# ------------------------------------------------------------------------------------------ corners (tests/golden/hinit_set)
RUNS = {"plain": ({}, []), "umv": (dict(uflags=1 | 2), ["-u", "mv"]), "vfloor": (dict(min_var=0.5), ["-v", "0.5"]),
        "wfloor": (dict(mix_weight_floor=9000 * 1.0e-5), ["-w", "9000"])}


def corner_data(native, tmp):
    from examples.hinit_set import tokens_from_labels
    lst = os.path.join(str(tmp), "list")
    open(lst, "w").write("A\nB\nC\n")
    mmf = native.Mmf(hmm_list=lst, hmm_dir=os.path.join(HSET, "proto"))
    z = np.load(os.path.join(HSET, "data.npz"))
    stat = [z["f%d" % i] for i in range(3)]
    labels = [native.labels_read(os.path.join(HSET, "labels", "f%d.lab" % i)) for i in range(3)]
    frame_off = np.concatenate([[0], np.cumsum([x.shape[0] for x in stat])]).astype(np.int32)
    pk = mmf.packed()
    return mmf, pk, stat, native.DevArray(np.ascontiguousarray(np.concatenate(stat), np.float32)), frame_off, tokens_from_labels(pk, mmf.logical, frame_off, labels), lst


@pytest.mark.parametrize("run", list(RUNS))
def test_corners_against_the_reference(native, tmp_path, run):
    from htk_amd import synth
    mmf, pk, stat, dX, frame_off, tok, lst = corner_data(native, tmp_path)
    lens = {n: tok[tok[:, 2] == mmf.logical[n], 1] for n in "ABC"}
    assert int(pk["hmmStateOff"][mmf.logical["A"] + 1] - pk["hmmStateOff"][mmf.logical["A"]]) == 5      # a 5-state model beside 3-state ones
    assert lens["A"].min() == 5 and lens["B"].min() == 3 and lens["C"].min() == 3                       # tokens exactly as long as the models
    kw, switches = RUNS[run]
    model, res = native.hinit(pk, dX.ptr, int(frame_off[-1]), tok, [mmf.logical[n] for n in "ABC"], native.hinit_config(max_iter=10, **kw))
    p, res = model.get_params(), dict(zip("ABC", res))
    refs = [os.path.join(HSET, run)]
    if os.path.exists(HINIT):                             # the reference on the spot as well
        out = tmp_path / "ref"; out.mkdir()
        data = []
        for i, X in enumerate(stat):
            data.append(str(tmp_path / ("f%d.usr" % i))); synth.write_htk_param(data[-1], X, kind=9)
        for n in "ABC":
            subprocess.run([HINIT, "-i", "10"] + switches + ["-L", os.path.join(HSET, "labels"), "-l", n, "-o", n, "-M", str(out), os.path.join(HSET, "proto", n)] + data,
                           check=True, stdout=subprocess.DEVNULL)
        refs.append(str(out))
    proto = native.Model(pk).get_params()
    for ref_dir in refs:
        rmmf = native.Mmf(hmm_list=lst, hmm_dir=ref_dir)
        rq = rmmf.packed()
        for n in "ABC":
            ref, converged = hu.ref_trace(os.path.join(HSET, run + ".log"), n)
            r = res[n]
            assert r["status"] == 0 and r["passes"] == len(ref) and r["converged"] == converged, (n, r, ref)
            for x, rx in zip(r["logP"], ref):
                assert abs(x - rx) <= 1e-6 * abs(rx), (n, r["logP"], ref)
            hu.compare_model(p, pk, mmf.logical[n], rq, rmmf.logical[n], weights=True)
        if run == "vfloor":                               # the floor binds in the reference's own output
            assert (rq["var"] == np.float32(0.5)).any() and (rq["var"] > np.float32(0.5)).any()
            assert (p["var"] == np.float32(0.5)).any()
        if run == "wfloor":
            # -w 9000 is a floor of 0.09.  HInit applies it to discrete sets only (UpDProbs HInit.c:1109; UpWeights :997 does not look at
            # it), so the reference's own output keeps a weight below it, and so does the library
            assert (rq["compWeight"] < 0.09).any() and (p["compWeight"] < 0.09).any()
    if run == "umv":                                      # transitions and weights are the prototype's bits
        assert np.array_equal(p["transP"].view(np.uint32), proto["transP"].view(np.uint32))
        assert np.array_equal(p["compWeight"].view(np.uint32), proto["compWeight"].view(np.uint32))
        assert not np.array_equal(p["mean"], proto["mean"])


# ------------------------------------------------------------------------------------------ the caller
def test_hinit_set_example_writes_the_same_models(native, demo_all, tmp_path):
    from examples import hinit_set
    files = sorted(os.path.join(hu.DEMO, "train", f) for f in os.listdir(os.path.join(hu.DEMO, "train")) if f.endswith(".mfc"))
    hinit_set.main(["--hmmlist", os.path.join(hu.DEMO, "bcplist"), "--hmmdir", os.path.join(hu.DEMO, "proto"), "--labdir", os.path.join(hu.DEMO, "labels"),
                    "--target-kind", "MFCC_E_D", "--maxiter", "10", "--outdir", str(tmp_path / "hmm0"), "--data"] + files)
    mmf, pk, p, res = demo_all
    got = native.Mmf(hmm_list=os.path.join(hu.DEMO, "bcplist"), hmm_dir=str(tmp_path / "hmm0"))
    gq = got.packed()
    for name in NAMES:
        hu.compare_model(p, pk, mmf.logical[name], gq, got.logical[name])
