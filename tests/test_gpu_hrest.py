"""HRest on the device (htk_amd/csrc/hrest.hip): every model of the demo in one call against the reference's traces and model files
(tests/golden/demo), the demo's mixture models and the corners of tests/golden/hrest_set against the reference's HRest, one call against
one call per model, per-model failures, maxIter = 1, and examples/hrest_set.py."""
import os
import re
import sys

import numpy as np
import pytest

import hinit_util as hu

pytestmark = pytest.mark.gpu

sys.path.insert(0, hu.ROOT)
NAMES = list("SCVNL")
HSET = os.path.join(hu.ROOT, "tests", "golden", "hinit_set")
RSET = os.path.join(hu.ROOT, "tests", "golden", "hrest_set")
DEMO_CFG = dict(min_var=0.05, mix_weight_floor=3 * 1.0e-5)          # the demo's HRest step: -v 0.05 -w 3 -i 10


def ref_trace(log_path, name):
    """[(Ave LogProb, examples used)] per pass and whether the reference converged, from the lines of one model"""
    lines = [l for l in open(log_path) if l.startswith("HRest %s:" % name)]
    ref = [(float(re.search(r"= +(-?[\d.]+) using", l).group(1)), int(re.search(r"using (\d+) examples", l).group(1))) for l in lines if "Ave LogProb" in l]
    return ref, any("converged" in l for l in lines)


def check_trace(r, ref, name):
    assert r["status"] == 0 and r["passes"] == len(ref) == len(r["logP"]), (name, r, ref)
    for k, (rp, rn) in enumerate(ref):
        print("%s pass %d: logP %.6f ref %.5f rel %.2e used %d ref %d" % (name, k + 1, r["logP"][k], rp, abs(r["logP"][k] - rp) / abs(rp), r["used"][k], rn))
    for k, (rp, rn) in enumerate(ref):
        assert r["used"][k] == rn and abs(r["logP"][k] - rp) <= 1e-6 * abs(rp), (name, k, r, ref)


# ------------------------------------------------------------------------------------------ the demo
def demo_data(native, hmm_dir):
    from examples.hinit_set import tokens_from_labels
    mmf = native.Mmf(hmm_list=os.path.join(hu.DEMO, "bcplist"), hmm_dir=hmm_dir)
    files = sorted(f for f in os.listdir(os.path.join(hu.DEMO, "train")) if f.endswith(".mfc"))
    stat = [native.parm_read(os.path.join(hu.DEMO, "train", f))[0] for f in files]
    labels = [native.labels_read(os.path.join(hu.DEMO, "labels", f.replace(".mfc", ".lab"))) for f in files]
    dX, frame_off, cols = native.parm_add_qualifiers(stat, hasD=True)                     # TARGETKIND = MFCC_E_D over the whole file
    pk = mmf.packed()
    assert cols == pk["vecSize"]
    return mmf, pk, dX, frame_off, tokens_from_labels(pk, mmf.logical, frame_off, labels, seg_reject=False)


@pytest.fixture(scope="module")
def demo(native):
    return demo_data(native, os.path.join(hu.DEMO, "hmm0"))


def run_demo(native, data, names=NAMES, model=None, **cfg):
    mmf, pk, dX, frame_off, tok = data
    model, res = native.hrest(model or pk, dX.ptr, int(frame_off[-1]), tok, [mmf.logical[n] for n in names], native.hrest_config(**cfg))
    return model, model.get_params(), dict(zip(names, res))


@pytest.fixture(scope="module")
def demo_all(native, demo):
    """SCVNL in ONE call with the reference's settings"""
    return run_demo(native, demo, max_iter=10, **DEMO_CFG)


def test_demo_all_models_in_one_call_stop_near_the_reference(native, demo_all):
    """the stopping pass depends on the last bits of a float near -600 (spacing 6e-5 against epsilon 1e-4): within 3 passes of the log's"""
    _, _, res = demo_all
    for name in NAMES:
        ref, _ = ref_trace(os.path.join(hu.DEMO, "hinit_hrest.log"), name)
        assert res[name]["status"] == 0 and abs(res[name]["passes"] - len(ref)) <= 3, (name, res[name], ref)


@pytest.fixture(scope="module")
def demo_by_passes(native, demo):
    """epsilon = 0 and maxIter = the reference's passes.  A call has one maxIter, so the models that the reference stopped at the same pass
    go into one call: one call per distinct pass count"""
    groups = {}
    for name in NAMES:
        groups.setdefault(len(ref_trace(os.path.join(hu.DEMO, "hinit_hrest.log"), name)[0]), []).append(name)
    out = {}
    for n, names in groups.items():
        _, p, res = run_demo(native, demo, names=names, max_iter=n, epsilon=0.0, **DEMO_CFG)
        for name in names:
            out[name] = (p, res[name])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_demo_pass_by_pass_and_final_models(native, demo, demo_by_passes, name):
    mmf, pk = demo[0], demo[1]
    p, r = demo_by_passes[name]
    ref, _ = ref_trace(os.path.join(hu.DEMO, "hinit_hrest.log"), name)
    check_trace(r, ref, name)
    assert not r["converged"]
    rmmf = native.Mmf(hmm_list=os.path.join(hu.DEMO, "bcplist"), hmm_dir=os.path.join(hu.DEMO, "hmm1"))
    hu.compare_model(p, pk, mmf.logical[name], rmmf.packed(), rmmf.logical[name])


@pytest.fixture(scope="module")
def demo_mix(native):
    data = demo_data(native, os.path.join(hu.DEMO, "hinit_mix", "hmm0"))
    return data, run_demo(native, data, max_iter=10, **DEMO_CFG)


@pytest.mark.parametrize("name", NAMES)
def test_demo_mixture_models_in_one_call(native, demo_mix, name):
    (mmf, pk, _, _, _), (_, p, res) = demo_mix
    ref, converged = ref_trace(os.path.join(RSET, "mix.log"), name)
    assert len(ref) == 10 and not converged              # every change of the tenth pass is far above epsilon: the stop is maxIter's
    check_trace(res[name], ref, name)
    assert res[name]["converged"] == converged
    rmmf = native.Mmf(hmm_list=os.path.join(hu.DEMO, "bcplist"), hmm_dir=os.path.join(RSET, "mix"))
    hu.compare_model(p, pk, mmf.logical[name], rmmf.packed(), rmmf.logical[name], weights=True)
    h = mmf.logical[name]
    assert [int(pk["stateCompOff"][s + 1] - pk["stateCompOff"][s]) for s in pk["hmmState"][pk["hmmStateOff"][h]:pk["hmmStateOff"][h + 1]]] == [2, 3, 2]


# ------------------------------------------------------------------------------------------ independence and freezing
@pytest.fixture(scope="module")
def demo_single(native, demo):
    return {name: run_demo(native, demo, names=[name], max_iter=10, **DEMO_CFG) for name in NAMES}


def test_models_stop_at_different_passes(demo_all):
    assert len({demo_all[2][n]["passes"] for n in NAMES}) >= 2           # (else nothing below sees a frozen model)


@pytest.mark.parametrize("name", NAMES)
def test_one_call_over_five_models_equals_a_call_per_model(native, demo, demo_all, demo_single, name):
    """The statistics are summed with atomic adds (forward-backward's accumulators), so their order is not fixed and the parameters are
    held to the bars of the reference comparison, not to bit equality; the counts and the stopping pass are equal."""
    mmf, pk = demo[0], demo[1]
    _, p, res = demo_all
    _, p1, res1 = demo_single[name]
    r, r1 = res[name], res1[name]
    assert (r["status"], r["passes"], r["converged"], r["used"]) == (r1["status"], r1["passes"], r1["converged"], r1["used"]) and r["status"] == 0
    for x, y in zip(r["logP"], r1["logP"]):
        assert abs(x - y) <= 1e-6 * abs(y), (name, r, r1)
    hu.compare_model(p, pk, mmf.logical[name], pk | p1, mmf.logical[name])      # a model frozen at pass k has the parameters of its own call
    start = native.Model(pk).get_params()                   # the call alone trained nothing else
    for other in NAMES:
        if other != name:
            assert hu.model_params_equal(p1, start, pk, mmf.logical[other]), other


# ------------------------------------------------------------------------------------------ corners (tests/golden/hrest_set)
RUNS = {"plain": {}, "umv": dict(uflags=1 | 2), "vfloor": dict(min_var=0.5), "wfloor": dict(mix_weight_floor=9000 * 1.0e-5)}


def corner_data(native, tmp, labels="labels", labdir=None):
    from examples.hinit_set import tokens_from_labels
    lst = os.path.join(str(tmp), "list")
    open(lst, "w").write("A\nB\nC\n")
    mmf = native.Mmf(hmm_list=lst, hmm_dir=os.path.join(RSET, "start"))
    z = np.load(os.path.join(HSET, "data.npz"))
    stat = [z["f%d" % i] for i in range(3)]
    labdir = labdir or os.path.join(HSET, "labels")
    labs = [native.labels_read(os.path.join(labdir, "f%d.lab" % i)) for i in range(3)]
    frame_off = np.concatenate([[0], np.cumsum([x.shape[0] for x in stat])]).astype(np.int32)
    pk = mmf.packed()
    tok = tokens_from_labels(pk, mmf.logical, frame_off, labs, seg_reject=False)
    return mmf, pk, native.DevArray(np.ascontiguousarray(np.concatenate(stat), np.float32)), frame_off, tok, lst


def check_corner(native, mmf, pk, p, res, names, run, lst, log=None):
    rmmf = native.Mmf(hmm_list=lst, hmm_dir=os.path.join(RSET, run))
    rq = rmmf.packed()
    for n in names:
        ref, converged = ref_trace(os.path.join(RSET, (log or run) + ".log"), n)
        check_trace(res[n], ref, n)
        assert res[n]["converged"] == converged
        hu.compare_model(p, pk, mmf.logical[n], rq, rmmf.logical[n], weights=True)
    return rq


@pytest.mark.parametrize("run", list(RUNS))
def test_corners_against_the_reference(native, tmp_path, run):
    mmf, pk, dX, frame_off, tok, lst = corner_data(native, tmp_path)
    model, res = native.hrest(pk, dX.ptr, int(frame_off[-1]), tok, [mmf.logical[n] for n in "ABC"], native.hrest_config(max_iter=10, **RUNS[run]))
    p, res = model.get_params(), dict(zip("ABC", res))
    rq = check_corner(native, mmf, pk, p, res, "ABC", run, lst)
    start = native.Model(pk).get_params()
    if run == "vfloor":                                   # the floor binds in the reference's own output, on one dimension
        assert (rq["var"][:, 3] == np.float32(0.5)).all() and (rq["var"][:, :3] > np.float32(0.5)).all()
        assert (p["var"][:, 3] == np.float32(0.5)).all() and (p["var"][:, :3] > np.float32(0.5)).all()
    if run == "wfloor":                                   # -w 9000 is a floor of 0.09: the rare component's weight was below it and is it now
        rare = int(np.argmin(start["compWeight"]))
        assert start["compWeight"][rare] < 0.08 and abs(rq["compWeight"][rare] - 0.09) < 1e-6 and abs(p["compWeight"][rare] - 0.09) < 1e-6
    if run == "umv":
        # transitions are the start's bits.  The weights are not re-estimated, but RestStream runs FloorMixes whatever -u says
        # (HRest.c:1270), which rescales them by 1 / their float sum: the reference's own umv/B has 4.615384e-01 where start/B has
        # 4.615385e-01.  So "untouched" is one rounding of the start's weights, not their bits
        assert np.array_equal(p["transP"].view(np.uint32), start["transP"].view(np.uint32))
        assert np.abs(p["compWeight"] - start["compWeight"]).max() <= 2.0e-7
        assert not np.array_equal(p["mean"], start["mean"])


def test_short_tokens_are_dropped_or_skipped_as_in_the_reference(native, tmp_path):
    mmf, pk, dX, frame_off, tok, lst = corner_data(native, tmp_path, labdir=os.path.join(RSET, "labels_short"))
    a = mmf.logical["A"]
    assert (tok[tok[:, 2] == a, 1] < 5).sum() == 1                   # one token of A is shorter than its five emitting states
    lst = os.path.join(str(tmp_path), "list_a")                      # (the reference's runs of this corner wrote A alone)
    open(lst, "w").write("A\n")
    for run, reject, loaded in (("short", True, 17), ("short_t", False, 18)):
        cfg = native.hrest_config(max_iter=10, seg_reject=reject)
        _, kept, _ = native.hrest_token_counts(pk, tok, cfg, [a])
        assert kept[0] == loaded
        assert ("%d Examples loaded" % loaded) in open(os.path.join(RSET, run + ".log")).read()
        model, res = native.hrest(pk, dX.ptr, int(frame_off[-1]), tok, [a], cfg)
        check_corner(native, mmf, pk, model.get_params(), {"A": res[0]}, "A", run, lst)
        assert res[0]["used"] == [17] * res[0]["passes"]


# ------------------------------------------------------------------------------------------ failures are per model
def test_too_few_tokens_is_that_models_status(native, tmp_path):
    mmf, pk, dX, frame_off, tok, lst = corner_data(native, tmp_path, labdir=os.path.join(RSET, "labels_few"))
    assert "ERROR [+2221]" in open(os.path.join(RSET, "few.log")).read()
    model, res = native.hrest(pk, dX.ptr, int(frame_off[-1]), tok, [mmf.logical[n] for n in "ABC"], native.hrest_config(max_iter=10, min_seg=3))
    p, res = model.get_params(), dict(zip("ABC", res))
    assert res["C"]["status"] == native.HREST_EFEWSEGS and res["C"]["passes"] == 0 and not res["C"]["converged"]
    assert hu.model_params_equal(p, native.Model(pk).get_params(), pk, mmf.logical["C"])
    check_corner(native, mmf, pk, p, res, "AB", "plain", lst)


def test_no_usable_token_is_that_models_status_and_the_handle_goes_on(native, tmp_path):
    mmf, pk, dX, frame_off, tok, lst = corner_data(native, tmp_path)
    b = mmf.logical["B"]
    t = int(pk["hmmTrans"][b]); N = int(pk["transN"][t]); o = int(pk["transOff"][t])
    pk = dict(pk); pk["transP"] = pk["transP"].copy()
    row = pk["transP"][o + N:o + 2 * N]                                # B's first emitting state: only its self-loop is left, no way on
    row[:] = np.float32(-1.0e10); row[1] = np.float32(0.0)
    cfg = native.hrest_config(max_iter=10)
    model, res = native.hrest(pk, dX.ptr, int(frame_off[-1]), tok, [mmf.logical[n] for n in "ABC"], cfg)
    p, res = model.get_params(), dict(zip("ABC", res))
    assert res["B"]["status"] == native.HREST_ENOUSABLE and res["B"]["passes"] == 0 and not res["B"]["converged"]
    assert hu.model_params_equal(p, native.Model(pk).get_params(), pk, b)
    check_corner(native, mmf, pk, p, res, "AC", "plain", lst)
    # a second call on the same handle: C again from where it stands (converged: one or two passes), B fails again, A is not named
    before = model.get_params()
    _, res2 = native.hrest(model, dX.ptr, int(frame_off[-1]), tok, [mmf.logical["C"], b], cfg)
    assert res2[0]["status"] == 0 and 1 <= res2[0]["passes"] <= 3 and res2[0]["converged"] and res2[1]["status"] == native.HREST_ENOUSABLE
    after = model.get_params()
    assert hu.model_params_equal(after, before, pk, mmf.logical["A"]) and hu.model_params_equal(after, before, pk, b)


def test_a_model_that_fails_in_a_later_pass_is_put_back_too(native, tmp_path):
    """VDEFUNCT above every variance.  A (single Gaussians) has a "Zero Covariance" in its first update: 2222 after no pass.  In B and C
    every component of every state goes defunct in the first update (-2225: weight 0, and FloorMixes with floor 0 leaves the zeros), so
    the SECOND pass finds no usable token: 2226 after one pass -- and the parameters are the start's bits, not the first update's."""
    mmf, pk, dX, frame_off, tok, lst = corner_data(native, tmp_path)
    model, res = native.hrest(pk, dX.ptr, int(frame_off[-1]), tok, [mmf.logical[n] for n in "ABC"], native.hrest_config(max_iter=10, v_defunct=1.0e9))
    p, res, start = model.get_params(), dict(zip("ABC", res)), native.Model(pk).get_params()
    assert res["A"]["status"] == native.HREST_EZEROOCC and res["A"]["passes"] == 0
    for n in "BC":
        ref, _ = ref_trace(os.path.join(RSET, "plain.log"), n)
        assert res[n]["status"] == native.HREST_ENOUSABLE and res[n]["passes"] == 1 and not res[n]["converged"], (n, res[n])
        assert res[n]["used"] == [ref[0][1]] and abs(res[n]["logP"][0] - ref[0][0]) <= 1e-6 * abs(ref[0][0])      # the first pass was a whole one
    for n in "ABC":
        assert hu.model_params_equal(p, start, pk, mmf.logical[n]), n
    # the scoring tables went back with them: the same handle trains as a fresh one does
    _, res2 = native.hrest(model, dX.ptr, int(frame_off[-1]), tok, [mmf.logical[n] for n in "ABC"], native.hrest_config(max_iter=10))
    check_corner(native, mmf, pk, model.get_params(), dict(zip("ABC", res2)), "ABC", "plain", lst)


def test_a_handle_with_tied_vectors_is_refused(native, tmp_path):
    """~u / ~v sharing is not part of a description, so this refusal is the call's own (htkamd_hrest_check cannot make it)"""
    mmf, pk, dX, frame_off, tok, lst = corner_data(native, tmp_path)
    pk = dict(pk); pk["var"] = pk["var"].copy(); pk["var"][1] = pk["var"][0]
    share = np.full(pk["var"].shape[0], -1, np.int32); share[:2] = 0
    model = native.Model(pk)
    model.set_sharing(np.full(len(share), -1, np.int32), share)
    before = model.get_params()
    with pytest.raises(native.HtkAmdError, match="hrest: a set with shared mean / variance vectors") as e:
        native.hrest(model, dX.ptr, int(frame_off[-1]), tok, [mmf.logical["A"]], native.hrest_config())
    assert e.value.rc == -5
    after = model.get_params()
    assert all(np.array_equal(before[k], after[k]) for k in ("mean", "var", "compWeight", "transP"))


def test_max_iter_one_is_one_pass_and_one_update(native, tmp_path):
    mmf, pk, dX, frame_off, tok, lst = corner_data(native, tmp_path)
    model, res = native.hrest(pk, dX.ptr, int(frame_off[-1]), tok, [mmf.logical[n] for n in "ABC"], native.hrest_config(max_iter=1))
    p, start = model.get_params(), native.Model(pk).get_params()
    for n, r in zip("ABC", res):
        ref, _ = ref_trace(os.path.join(RSET, "plain.log"), n)
        assert r["status"] == 0 and r["passes"] == 1 and not r["converged"] and r["used"] == [ref[0][1]]
        assert abs(r["logP"][0] - ref[0][0]) <= 1e-6 * abs(ref[0][0])
        assert not hu.model_params_equal(p, start, pk, mmf.logical[n])          # updated ...
    # ... once: the second pass of a two-pass run starts from these parameters, so its first log probability is that run's second
    _, res2 = native.hrest(model, dX.ptr, int(frame_off[-1]), tok, [mmf.logical[n] for n in "ABC"], native.hrest_config(max_iter=1))
    for n, r in zip("ABC", res2):
        ref, _ = ref_trace(os.path.join(RSET, "plain.log"), n)
        assert abs(r["logP"][0] - ref[1][0]) <= 1e-6 * abs(ref[1][0]), (n, r, ref)


# ------------------------------------------------------------------------------------------ the caller
@pytest.fixture(scope="module")
def example_run(native, tmp_path_factory):
    import contextlib
    import io
    from examples import hrest_set
    out = tmp_path_factory.mktemp("hrest_set") / "hmm1"
    files = sorted(os.path.join(hu.DEMO, "train", f) for f in os.listdir(os.path.join(hu.DEMO, "train")) if f.endswith(".mfc"))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model, res = hrest_set.main(["--hmmlist", os.path.join(hu.DEMO, "bcplist"), "--hmmdir", os.path.join(hu.DEMO, "hmm0"), "--labdir", os.path.join(hu.DEMO, "labels"),
                                     "--target-kind", "MFCC_E_D", "-i", "10", "-v", "0.05", "-w", "3", "-T", "1", "-o", str(out), "--data"] + files)
    return str(out), model.get_params(), res, buf.getvalue()


def test_hrest_set_example_writes_the_models_the_call_returned(native, demo, example_run):
    mmf, pk = demo[0], demo[1]
    out, p, res, _ = example_run
    assert all(r["status"] == 0 for r in res)
    got = native.Mmf(hmm_list=os.path.join(hu.DEMO, "bcplist"), hmm_dir=out)
    gq = got.packed()
    for name in NAMES:
        hu.compare_model(p, pk, mmf.logical[name], gq, got.logical[name])


def test_hrest_set_example_prints_the_references_lines(example_run):
    _, _, res, text = example_run
    lines = text.splitlines()
    first = re.compile(r"^HRest [SCVNL]: Ave LogProb at iter 1 = [ -]\d{3}\.\d{5} using \d+ examples$")
    later = re.compile(r"^HRest [SCVNL]: Ave LogProb at iter \d+ = [ -]\d{3}\.\d{5} using \d+ examples  change = [ -]{1,4}\d+\.\d{5}$")
    end = re.compile(r"^HRest [SCVNL]: Estimation (converged|aborted) at iteration \d+$")
    assert len(lines) == sum(r["passes"] for r in res) + 5
    assert sum(bool(first.match(l)) for l in lines) == 5 and sum(bool(end.match(l)) for l in lines) == 5
    assert all(first.match(l) or later.match(l) or end.match(l) for l in lines), [l for l in lines if not (first.match(l) or later.match(l) or end.match(l))]
    # the same patterns take every line of the reference's own log
    ref = [l.rstrip("\n") for l in open(os.path.join(hu.DEMO, "hinit_hrest.log")) if l.startswith("HRest")]
    assert ref and all(first.match(l) or later.match(l) or end.match(l) for l in ref)
