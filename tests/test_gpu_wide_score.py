"""HTKAMD_SCORE_BF16 on wide feature vectors (46 <= D <= 120: gmm_bf16x.hip) against a float64 evaluation of the packed model."""
import numpy as np
import pytest

from util import batch_arrays

pytestmark = pytest.mark.gpu

LMINMIX = -11.5129254649702


def ref64(pk, X, states):
    """log sum_m w_m N(x; mu_m, var_m) in float64, [T, len(states)]; a mixture's components at or below LMINMIX are left out."""
    X = np.asarray(X, np.float64)
    mean, var = np.asarray(pk["mean"], np.float64), np.asarray(pk["var"], np.float64)
    out = np.empty((X.shape[0], len(states)))
    for i, s in enumerate(states):
        c0, c1 = int(pk["stateCompOff"][s]), int(pk["stateCompOff"][s + 1])
        terms = []
        for c in range(c0, c1):
            w = float(pk["compWeight"][c])
            lw = 0.0 if c1 - c0 == 1 else (np.log(w) if w > 0 else -np.inf)
            if c1 - c0 > 1 and lw <= LMINMIX:
                continue
            g = int(pk["compGauss"][c])
            gconst = X.shape[1] * np.log(2 * np.pi) + np.log(var[g]).sum()
            terms.append(lw - 0.5 * (gconst + ((X - mean[g]) ** 2 / var[g]).sum(axis=1)))
        out[:, i] = np.logaddexp.reduce(np.array(terms), axis=0)
    return out


def check_block(native, oracle, pk, X, T_extra):
    gm = native.Model(pk)
    states = np.arange(int(pk["numStates"]), dtype=np.int32)[::-1].copy()
    ref = ref64(pk, X, states)
    for Xs, r in ((X, ref), (X[:T_extra], ref[:T_extra])):
        new, exact = gm.outp_block(Xs, states, mode=4), gm.outp_block(Xs, states, mode=0)
        assert new.shape == r.shape and np.isfinite(new).all()
        if Xs is X:
            assert np.array_equal(exact, oracle.Model(pk).score_block(X, states))      # the exact mode is untouched
        e_new, e_exact = np.abs(new - r), np.abs(exact - r)
        print("T=%d e_new max %.3g mean %.3g   e_exact max %.3g mean %.3g" % (len(Xs), e_new.max(), e_new.mean(), e_exact.max(), e_exact.mean()))
        assert e_new.max() <= max(1e-3, 2 * e_exact.max()), (e_new.max(), e_exact.max())
        assert e_new.mean() <= max(1e-4, 2 * e_exact.mean()), (e_new.mean(), e_exact.mean())


@pytest.mark.parametrize("D,M,T_extra", [(46, 3, 1), (60, 16, 16), (61, 1, 17), (78, 17, 129), (120, 33, 17), (120, 2, 129)])
def test_wide_block_scores_against_fp64(native, oracle, D, M, T_extra):
    """46: first size past the old limit, NC = 4 with a ragged last chunk; 60: four full chunks; 61: NC = 5, single Gaussians;
    M = 17 / 33 cross tile edges; 120: every chunk full at the maximum.  T = 150 is two frame tiles; 1 / 16 / 17 / 129 are the
    column-tile and frame-tile edges.  The bound: the project's tolerance class, or twice the exact kernel's own distance from fp64."""
    from htk_amd import synth
    s = synth.generate(25, M, 10, 1, 150, 900 + D + M, D=D)
    check_block(native, oracle, s.packed(), s.feats[0], T_extra)


def test_wide_dead_component(native, oracle):
    """A component of weight 0 contributes nothing (its table row starts at -1e30)."""
    from htk_amd import synth
    s = synth.generate(25, 4, 10, 1, 150, 982, D=78)
    pk = s.packed()
    pk["compWeight"] = pk["compWeight"].copy()
    pk["compWeight"][4 * 7 + 2] = 0.0
    check_block(native, oracle, pk, s.feats[0], 17)


@pytest.mark.parametrize("D,mode,runs", [(121, 4, False), (52, 32, False), (45, 4, True)])
def test_wide_limits(native, D, mode, runs):
    from htk_amd import synth
    s = synth.generate(6, 2, 4, 1, 20, 5, D=D)
    gm = native.Model(s.packed())
    states = np.arange(6, dtype=np.int32)
    if runs:
        assert np.abs(gm.outp_block(s.feats[0], states, mode=mode) - gm.outp_block(s.feats[0], states, mode=0)).max() <= 1e-3
    else:
        with pytest.raises(native.HtkAmdError):
            gm.outp_block(s.feats[0], states, mode=mode)


def test_wide_forward_backward_and_device_update(native):
    """D = 52: a pass in bf16 x 3 scores + fast LAdd and the device update against the same in the exact mode (the parameter bars of
    test_mfma_forward_backward_within_tolerance), then a second pass on the updated model: its table was rebuilt."""
    from htk_amd import synth
    s = synth.generate(12, 3, 8, 12, 72, 31, D=52)      # 864 frames for 36 Gaussians: no variance collapses in the update
    pk = s.packed()
    X, frameOff, labOff, labs = batch_arrays([dict(seq=q, feat=x) for q, x in zip(s.seqs, s.feats)])
    dX = native.DevArray(X)

    def one_pass(model, mode, update):
        fb, acc = native.ForwardBackward(model), native.Accs(model)
        fb.prepare(dX.ptr.value, frameOff, labOff, labs)
        fb.execute(native.fb_config(scoreMode=mode), acc)
        pr, st = fb.results()
        assert (st == 1).all()
        occ = acc.download()["muOcc"]
        if update:
            model.update_device(acc, minEgs=1, minVar=0.01)
        return pr, np.asarray(occ, np.float64)

    mx, mb = native.Model(pk), native.Model(pk)
    pr_x, occ = one_pass(mx, 0, True)
    pr_b, _ = one_pass(mb, native.SCORE_BF16 | native.SCORE_FASTLADD, True)
    assert np.allclose(pr_b, pr_x, rtol=1e-6, atol=0)
    px, pb = mx.get_params(), mb.get_params()
    ref_mean, ref_var = px["mean"].astype(np.float64), px["var"].astype(np.float64)
    assert (np.abs(pb["mean"] - ref_mean) <= 1e-4 * np.maximum(np.abs(ref_mean), np.sqrt(ref_var)) + 1e-6).all()
    well = np.broadcast_to((occ >= 2.0)[:, None], ref_var.shape)
    assert well.sum() > 0.3 * well.size
    assert np.allclose(pb["var"][well], ref_var[well], rtol=1e-4, atol=1e-6)
    moment = ref_var + (ref_mean - np.asarray(pk["mean"], np.float64)) ** 2
    assert (np.abs(pb["var"] - ref_var)[~well] <= 1e-4 * moment[~well] + 1e-6).all()
    assert np.allclose(pb["compWeight"], px["compWeight"], rtol=1e-4, atol=2e-6)
    assert (pb["mean"] != np.asarray(pk["mean"], np.float32)).any()
    # the second pass: the updated model in the bf16 mode against the SAME model in the exact mode
    pr_b2, _ = one_pass(mb, native.SCORE_BF16 | native.SCORE_FASTLADD, False)
    pr_x2, _ = one_pass(mb, 0, False)
    assert np.allclose(pr_b2, pr_x2, rtol=1e-6, atol=0) and (pr_b2 != pr_b).all()
