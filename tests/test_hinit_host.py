"""HInit on the device, the parts that need no device (htk_amd/host/hinit.c, htk_amd/capi.py): the symbols and the wrappers' arguments,
every refusal by reason and return code before a device is looked for, the no-device error, and the host twin of the pool listing
against the per-model example's rule."""
import ctypes as C
import os

import numpy as np
import pytest

import hinit_util as hu

EINVAL, ENODEV, EMODEL = -1, -2, -5


def toy_set(n_models=3, n_emit=3, M=2, D=4):
    """a packed description of n_models left-to-right models, nothing shared"""
    S = n_models * n_emit
    N = n_emit + 2
    tp = np.full((N, N), -1.0e10, np.float32)
    tp[0, 1] = 0.0
    for i in range(1, N - 1):
        tp[i, i] = np.log(0.6); tp[i, i + 1] = np.log(0.4)
    return dict(vecSize=D, numStates=S, numComp=S * M, numGauss=S * M, numTrans=n_models, numPhys=n_models,
                stateCompOff=np.arange(S + 1, dtype=np.int32) * M, compWeight=np.full(S * M, 1.0 / M, np.float32), compGauss=np.arange(S * M, dtype=np.int32),
                mean=np.zeros((S * M, D), np.float32), var=np.ones((S * M, D), np.float32), gconst=None,
                transN=np.full(n_models, N, np.int32), transOff=np.arange(n_models + 1, dtype=np.int32) * N * N, transP=np.tile(tp.reshape(-1), n_models),
                hmmTrans=np.arange(n_models, dtype=np.int32), hmmStateOff=np.arange(n_models + 1, dtype=np.int32) * n_emit, hmmState=np.arange(S, dtype=np.int32))


TOKENS = [(0, 6, 0), (6, 6, 1), (12, 6, 2), (18, 6, 0), (24, 6, 1), (30, 6, 2), (36, 6, 0), (42, 6, 1), (48, 6, 2)]


def test_symbols_and_wrappers(native):
    L = native.lib()
    for f in ("htkamd_hinit", "htkamd_hinit_check", "htkamd_hinit_uniform_states", "htkamd_flat_cluster"):
        assert hasattr(L, f), f
    cfg = native.hinit_config()
    assert (cfg.maxIter, cfg.minSeg, cfg.uFlags, cfg.newModel) == (20, 3, native.UPALL, 1)
    assert abs(cfg.epsilon - 1.0e-4) < 1e-10 and abs(cfg.minVar - 1.0e-2) < 1e-9 and cfg.mixWeightFloor == 0.0
    cfg = native.hinit_config(max_iter=7, epsilon=0.5, min_var=0.25, min_seg=2, mix_weight_floor=3 * native.MINMIX, uflags=native.UPMEANS | native.UPVARS, new_model=False)
    assert (cfg.maxIter, cfg.epsilon, cfg.minVar, cfg.minSeg, cfg.uFlags, cfg.newModel) == (7, 0.5, 0.25, 2, 3, 0) and abs(cfg.mixWeightFloor - 3.0e-5) < 1e-10
    assert C.sizeof(native.HInitConfig) == 28
    assert (native.HINIT_EFEWSEGS, native.HINIT_ESHORT, native.HINIT_ENOPATH, native.HINIT_EZEROOCC, native.HINIT_ECLUSTER) == (2121, 2122, 2126, 2127, 7120)
    native.hinit_check(toy_set(), 54, TOKENS, native.hinit_config(), [0, 1, 2])          # nothing to refuse


def refused(native, reason, rc, pk=None, n_frames=54, tokens=TOKENS, models=(0, 1, 2), **cfg):
    """through the check alone and through the whole call: the reason arrives either way, and before a device is looked for"""
    for call in (lambda: native.hinit_check(pk or toy_set(), n_frames, tokens, native.hinit_config(**cfg), list(models)),
                 lambda: native.hinit(pk or toy_set(), None, n_frames, tokens, list(models), native.hinit_config(**cfg))):
        with pytest.raises(native.HtkAmdError, match=reason) as e:
            call()
        assert e.value.rc == rc


def test_sets_that_are_refused(native):
    pk = toy_set(); pk["var"] = None
    refused(native, "a FULLC set", EMODEL, pk=pk)
    pk = toy_set(); pk["hsKind"] = 1
    refused(native, "a tied-mixture set", EMODEL, pk=pk)
    pk = toy_set(); pk["numStreams"] = 2; pk["dimStream"] = np.array([0, 0, 1, 1], np.int32)
    refused(native, "a set of 2 streams", EMODEL, pk=pk)


def test_shared_structure_among_the_models_is_refused(native):
    pk = toy_set(); pk["hmmState"] = pk["hmmState"].copy(); pk["hmmState"][3] = 0          # model 1's first state is model 0's
    refused(native, "state 0 is shared by models to be trained \\(model 1\\): HInit trains in isolation", EMODEL, pk=pk)
    native.hinit_check(pk, 54, TOKENS, native.hinit_config(), [1, 2])                      # (fine when only one of the two is trained)
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
    refused(native, "update flags 16", EINVAL, uflags=16)


def test_without_a_device_the_call_ends_in_no_hip_device(native):
    if native.lib().htkamd_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(native.HtkAmdError, match="no HIP device") as e:
        native.hinit(toy_set(), None, 54, TOKENS, [0, 1, 2])
    assert e.value.rc == ENODEV
    X = np.zeros((8, 4), np.float32)
    with pytest.raises(native.HtkAmdError, match="flat_cluster: no HIP device") as e:
        native.flat_cluster(C.c_void_p(X.ctypes.data), 8, 4, [np.arange(8)], [2])
    assert e.value.rc == ENODEV


def test_flat_cluster_refusals_come_before_the_device(native):
    X = np.zeros((8, 4), np.float32)
    ptr = C.c_void_p(X.ctypes.data)
    with pytest.raises(native.HtkAmdError, match="item 3 is row 8 of 8") as e:
        native.flat_cluster(ptr, 8, 4, [np.array([0, 1, 2, 8])], [2])
    assert e.value.rc == EINVAL
    with pytest.raises(native.HtkAmdError, match="pool 1 asks for 0 clusters") as e:
        native.flat_cluster(ptr, 8, 4, [np.arange(4), np.arange(4, 8)], [2, 0])
    assert e.value.rc == EINVAL
    with pytest.raises(native.HtkAmdError, match="do not fit the workgroup's LDS") as e:
        native.flat_cluster(ptr, 8, 4000, [np.arange(2)], [200])
    assert e.value.rc == EINVAL


@pytest.mark.parametrize("n_emit", [1, 3, 5])
def test_pool_listing_is_the_examples_rule(native, n_emit):
    """tokens of N-2, N-1 and 2(N-2)+1 frames (and a spread of others): the state of every frame as examples/hinit_model.py::hinit has it,
    idx = (arange(L, float32) / (float32(L) / float32(ne))).astype(int32), and the pools in token order, then frame order"""
    lens = [n_emit, n_emit + 1, 2 * n_emit + 1] + list(range(n_emit, n_emit + 40)) + [97, 1000]
    got = native.hinit_uniform_states(n_emit, lens)
    want = np.concatenate([(np.arange(L, dtype=np.float32) / (np.float32(L) / np.float32(n_emit))).astype(np.int32) for L in lens])
    assert np.array_equal(got, want)
    at = 0
    for L in lens:
        s = got[at:at + L]; at += L
        assert s[0] == 0 and s[-1] == n_emit - 1 and (np.diff(s) >= 0).all() and set(s) == set(range(n_emit))     # every state gets frames, in order
    with pytest.raises(native.HtkAmdError, match="segment too short"):
        native.hinit_uniform_states(n_emit + 1, [n_emit])
