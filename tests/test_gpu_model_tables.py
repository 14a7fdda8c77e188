"""The model's derived scoring tables (fp32 fragments, bf16 x 3, fp16 x 2): built by the device builders alone, and current after
every change of the parameters.  Everything goes through htkamd_outp_block_mode on one task of 40 frames, over the two tiny sets of
tests/golden/make_model_tables_golden.py (W: D = 39, states of 1, 3, 16, 16 components, a dead column; N: D = 10, states of 1, 17, 5)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_tables")
PK_KEYS = ("vecSize", "numStates", "numComp", "numGauss", "stateCompOff", "compWeight", "compGauss", "mean", "var", "numTrans", "transN",
           "transOff", "transP", "numPhys", "hmmTrans", "hmmStateOff", "hmmState")
MODES = {"exact": 0, "mfma": 1, "bf16": 4, "f16": 32}          # HTKAMD_SCORE_*
OTHER = {"exact": "mfma", "mfma": "bf16", "bf16": "f16", "f16": "mfma"}
CHANGES = ("set_params", "set_prepared", "host_update", "device_update_scored", "device_update_unscored", "device_update_other_first", "set_compat")
_loaded = {}


def load(name):
    if name not in _loaded:
        z = np.load(os.path.join(GOLD, name + ".npz"))
        ld = {k: z[k] for k in z.files}
        ld["pk"] = {k: (int(ld[k]) if ld[k].ndim == 0 else ld[k]) for k in PK_KEYS}
        _loaded[name] = ld
    return _loaded[name]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def set_prepared(native, m, ivar, gconst, compLogWt):
    a = [np.ascontiguousarray(v, np.float32) for v in (ivar, gconst, compLogWt)]
    native.check(native.lib().htkamd_model_set_prepared(m.h, *[v.ctypes.data_as(C.c_void_p) for v in a]), "model_set_prepared")


@pytest.mark.parametrize("name", ["W", "N"])
def test_device_builder_equals_recorded_host_builder(native, name):
    """Test A: the HTKAMD_SCORE_MFMA scores of a freshly created model are, bit for bit, those recorded while the fp32 fragment table of
    a new model was still built by the host loop."""
    ld = load(name)
    m = native.Model(ld["pk"])
    got = m.outp_block(ld["X"], np.arange(m.S, dtype=np.int32), native.SCORE_MFMA)
    m.close()
    diff = np.abs(got.astype(np.float64) - ld["mfma"])
    print(name, "differing scores:", int((got.view(np.uint32) != ld["mfma"].view(np.uint32)).sum()), "of", got.size, "max |diff|", diff.max())
    assert same_bits(got, ld["mfma"])


def stats_vector(native, m, acc, ld):
    """An accumulator vector from the recorded statistics: means, variances and weights of every Gaussian, five examples per model."""
    pk, L = ld["pk"], acc.lay
    v = np.zeros(L.total, np.float64)
    G, D = m.G, m.D
    v[L.mu:L.mu + G * D] = ld["stat_mu"].reshape(-1); v[L.va:L.va + G * D] = ld["stat_va"].reshape(-1)
    v[L.muOcc:L.muOcc + G] = ld["stat_occ"]; v[L.vaOcc:L.vaOcc + G] = ld["stat_occ"]
    wt = ld["stat_occ"][pk["compGauss"]]
    v[L.wt:L.wt + m.C] = wt
    v[L.wtOcc:L.wtOcc + m.S] = np.add.reduceat(wt, pk["stateCompOff"][:-1])
    v[L.nEgs:L.nEgs + m.H] = 5
    return v


UPD = dict(minEgs=1, minVar=0.01, uFlags=1 | 2 | 8)            # means, variances, mixture weights


# (set_compat on the variant of W alone: N has no second state to share a Gaussian with)
CASES = [(n, mo, ch) for n in ("W", "N") for mo in MODES for ch in CHANGES if ch != "set_compat" or n == "W"]


@pytest.mark.parametrize("name,mode,change", CASES)
def test_tables_follow_every_parameter_change(native, name, mode, change):
    """Test B: after each way of changing the parameters, scoring in `mode` equals, bit for bit, scoring a second model that was given
    the changed model's floats (its means, and its prepared tables as the device holds them) and derived nothing itself."""
    ld = load(name)
    pk = dict(ld["pk"])
    if change == "set_compat":
        cg = pk["compGauss"].copy()
        cg[pk["stateCompOff"][3]] = cg[pk["stateCompOff"][2]]          # the two 16-component states list the same Gaussian first
        pk["compGauss"] = cg
    X, states, sm = ld["X"], np.arange(pk["numStates"], dtype=np.int32), MODES[mode]
    m = native.Model(pk)
    if change not in ("device_update_unscored", "device_update_other_first"):
        m.outp_block(X, states, sm)                                   # the path is in use and its table built before the change
    if change == "set_params":
        m.set_params(mean=pk["mean"] + np.float32(0.25), var=pk["var"] * np.float32(1.25))
    elif change == "set_prepared":
        q = m.get_prepared()
        set_prepared(native, m, q["ivar"] * np.float32(0.8), q["gconst"] + np.float32(1.0), q["compLogWt"] - np.float32(0.1))
    elif change == "set_compat":
        m.set_compat(native.COMPAT_SHARED_LOGWT)
    else:
        acc = native.Accs(m)
        vec = stats_vector(native, m, acc, dict(ld, pk=pk))
        if change == "host_update":
            m.update(acc, vec, **UPD)
        else:
            acc.upload_add(vec)
            m.update_device(acc, **UPD)
        acc.close()
    if change == "device_update_other_first":
        m.outp_block(X, states, MODES[OTHER[mode]])
    got = m.outp_block(X, states, sm)
    w = native.Model(pk)
    w.set_params(mean=m.get_params()["mean"])
    q = m.get_prepared()
    set_prepared(native, w, q["ivar"], q["gconst"], q["compLogWt"])
    want = w.outp_block(X, states, sm)
    f = native.Model(pk)
    fresh = f.outp_block(X, states, sm)
    m.close(); w.close(); f.close()
    print(name, mode, change, "differing scores:", int((got.view(np.uint32) != want.view(np.uint32)).sum()), "of", got.size)
    assert not same_bits(want, fresh), "the change did not change the scores: the case checks nothing"
    assert same_bits(got, want)
