"""HRest on the device, the parts that need no device (htk_amd/host/hrest.c, htk_amd/capi.py): the symbols and the wrappers' arguments,
every refusal by reason and return code before a device is looked for, the no-device error, and the short-token rejection with the -m
count on descriptions alone."""
import ctypes as C

import numpy as np
import pytest

from test_hinit_host import TOKENS, toy_set

EINVAL, ENODEV, EMODEL = -1, -2, -5


def test_symbols_and_wrappers(native):
    L = native.lib()
    for f in ("htkamd_hrest", "htkamd_hrest_check", "htkamd_hrest_token_counts"):
        assert hasattr(L, f), f
    cfg = native.hrest_config()
    assert (cfg.maxIter, cfg.minSeg, cfg.uFlags, cfg.segReject) == (20, 3, native.UPALL, 1)
    assert abs(cfg.epsilon - 1.0e-4) < 1e-10 and cfg.minVar == 0.0 and cfg.mixWeightFloor == 0.0 and cfg.vDefunct == 0.0
    cfg = native.hrest_config(max_iter=7, epsilon=0.5, min_var=0.25, min_seg=2, mix_weight_floor=3 * native.MINMIX, uflags=native.UPMEANS | native.UPVARS, seg_reject=False, v_defunct=0.125)
    assert (cfg.maxIter, cfg.epsilon, cfg.minVar, cfg.minSeg, cfg.uFlags, cfg.segReject, cfg.vDefunct) == (7, 0.5, 0.25, 2, 3, 0, 0.125) and abs(cfg.mixWeightFloor - 3.0e-5) < 1e-10
    assert C.sizeof(native.HRestConfig) == 32
    assert (native.HREST_EFEWSEGS, native.HREST_EZEROOCC, native.HREST_EFLOORSUM, native.HREST_ENOUSABLE) == (2221, 2222, 2223, 2226)
    native.hrest_check(toy_set(), 54, TOKENS, native.hrest_config(), [0, 1, 2])          # nothing to refuse


def refused(native, reason, rc, pk=None, n_frames=54, tokens=TOKENS, models=(0, 1, 2), **cfg):
    """through the check alone and through the whole call: the reason arrives either way, and before a device is looked for"""
    for call in (lambda: native.hrest_check(pk or toy_set(), n_frames, tokens, native.hrest_config(**cfg), list(models)),
                 lambda: native.hrest(pk or toy_set(), None, n_frames, tokens, list(models), native.hrest_config(**cfg))):
        with pytest.raises(native.HtkAmdError, match=reason) as e:
            call()
        assert e.value.rc == rc


def test_sets_that_are_refused(native):
    pk = toy_set(); pk["var"] = None
    refused(native, "hrest: a FULLC set", EMODEL, pk=pk)
    pk = toy_set(); pk["hsKind"] = 1
    refused(native, "hrest: a tied-mixture set", EMODEL, pk=pk)
    pk = toy_set(); pk["numStreams"] = 2; pk["dimStream"] = np.array([0, 0, 1, 1], np.int32)
    refused(native, "hrest: a set of 2 streams", EMODEL, pk=pk)


def test_a_discrete_set_is_refused(native):
    pk = toy_set(); pk["hsKind"] = 2
    refused(native, "hrest: a discrete set", EMODEL, pk=pk)


def test_shared_structure_among_the_models_is_refused(native):
    pk = toy_set(); pk["hmmState"] = pk["hmmState"].copy(); pk["hmmState"][3] = 0          # model 1's first state is model 0's
    refused(native, "state 0 is shared by models to be trained \\(model 1\\): HRest trains in isolation", EMODEL, pk=pk)
    native.hrest_check(pk, 54, TOKENS, native.hrest_config(), [1, 2])                      # (fine when only one of the two is trained)
    pk = toy_set(); pk["hmmState"] = pk["hmmState"].copy(); pk["hmmState"][1] = 0          # a state twice WITHIN model 0
    refused(native, "state 0 is shared by models to be trained \\(model 0\\)", EMODEL, pk=pk)
    pk = toy_set(); pk["compGauss"] = pk["compGauss"].copy(); pk["compGauss"][7] = 0       # a Gaussian of model 1 is model 0's
    refused(native, "Gaussian 0 is shared by models to be trained", EMODEL, pk=pk)
    pk = toy_set(); pk["hmmTrans"] = np.array([0, 1, 1], np.int32)
    refused(native, "transition matrix 1 is shared by models to be trained \\(model 2\\)", EMODEL, pk=pk)


def test_bad_lists_tokens_and_switches_are_refused(native):
    refused(native, "token 2 \\(frames 12 .. 17\\) lies outside the table of 15 frames", EINVAL, n_frames=15)
    refused(native, "token 0 \\(frames -1 .. 4\\) lies outside the table", EINVAL, tokens=[(-1, 6, 0)] + TOKENS[1:])
    refused(native, "token 1 names physical model 9 of 3", EINVAL, tokens=[TOKENS[0], (6, 6, 9)])
    refused(native, "physical model 1 is named twice", EINVAL, models=(0, 1, 1))
    refused(native, "names physical model 3 of 3", EINVAL, models=(0, 3))
    refused(native, "maxIter 0", EINVAL, max_iter=0)
    refused(native, "minSeg 0", EINVAL, min_seg=0)
    refused(native, "update flags 16", EINVAL, uflags=16)


def test_without_a_device_the_call_ends_in_no_hip_device(native):
    if native.lib().htkamd_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(native.HtkAmdError, match="no HIP device") as e:
        native.hrest(toy_set(), None, 54, TOKENS, [0, 1, 2])
    assert e.value.rc == ENODEV


def test_short_tokens_and_the_minimum_count(native):
    """three models of 3 emitting states; tokens of 2, 3 and 4 frames.  With rejection a 2-frame token is dropped before the -m count
    (LoadFile HRest.c:500, main :295); with -t it is kept and counted; tokens of unlisted models belong to nobody."""
    pk = toy_set()
    tok = [(0, 3, 0), (3, 2, 0), (5, 4, 0), (9, 2, 0),          # model 0: two of four survive
           (11, 3, 1), (14, 3, 1), (17, 3, 1), (20, 2, 1),      # model 1: three of four
           (22, 4, 2), (26, 4, 2), (30, 4, 2)]                  # model 2: not listed below
    keep, kept, status = native.hrest_token_counts(pk, tok, native.hrest_config(min_seg=3), [0, 1])
    assert list(keep) == [True, False, True, False, True, True, True, False, False, False, False]
    assert list(kept) == [2, 3] and list(status) == [native.HREST_EFEWSEGS, native.HREST_OK]
    keep, kept, status = native.hrest_token_counts(pk, tok, native.hrest_config(min_seg=3, seg_reject=False), [0, 1])
    assert list(keep) == [True] * 8 + [False] * 3 and list(kept) == [4, 4] and list(status) == [0, 0]
    keep, kept, status = native.hrest_token_counts(pk, tok, native.hrest_config(min_seg=4), [1, 2, 0])       # the list's order is the answer's
    assert list(kept) == [3, 3, 2] and list(status) == [native.HREST_EFEWSEGS] * 3
    _, kept, status = native.hrest_token_counts(pk, tok, native.hrest_config(min_seg=2), [0])
    assert list(kept) == [2] and list(status) == [0]
    # a model of 5 emitting states beside them: the rule is per model
    pk5 = toy_set(n_models=1, n_emit=5)
    _, kept, _ = native.hrest_token_counts(pk5, [(0, 4, 0), (4, 5, 0), (9, 6, 0)], native.hrest_config(), [0])
    assert list(kept) == [2]


def test_the_example_refuses_a_set_with_a_variance_floor_macro(native, tmp_path):
    """SetVFloor (HModel.c:3512) would floor with ~v varFloor1; the call floors with -v alone, so the caller says so instead of
    flooring differently from the reference on the same files"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from examples import hrest_set
    demo = os.path.join(root, "tests", "golden", "demo")
    macros = tmp_path / "macros"                            # the global options, then what HCompV -f wrote for the demo's files
    macros.write_text("~o <VecSize> 26 <MFCC_E_D>\n" + open(os.path.join(root, "tests", "golden", "compv", "vFloors")).read())
    with pytest.raises(SystemExit, match="varFloor1"):
        hrest_set.main(["--hmmlist", os.path.join(demo, "bcplist"), "--mmf", str(macros), "--hmmdir", os.path.join(demo, "hmm0"),
                        "-o", str(tmp_path), "--data", os.path.join(demo, "train", "tr1.mfc")])
