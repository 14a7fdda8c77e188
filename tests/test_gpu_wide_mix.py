"""Mixture statistics by tied state for any vector size up to 128 and any mixture size (k_mixstate_x, fb_mixwide.hip) against the
C oracle's double accumulators, at the bars of test_gpu_parity.py."""
import numpy as np
import pytest

from util import acc_close, batch_arrays

pytestmark = pytest.mark.gpu

KEYS = ("mu", "muOcc", "va", "vaOcc", "wt", "wtOcc")


def make_set(D, M):
    """Three tied states under 1800 frames: the occupations of a frame sum to one, so one state holds more than 4 x 128 pairs."""
    from htk_amd import synth
    s = synth.generate(3, M, 2, 3, 600, 503 + D + M, D=D)
    return s.packed(), [dict(seq=q, feat=x) for q, x in zip(s.seqs, s.feats)]


def gpu_pass(native, pk, utts, uFlags=15, scoreMode=2, two_phase=False):
    model = native.Model(pk)
    X, frameOff, labOff, labs = batch_arrays(utts)
    dX = native.DevArray(X)
    fb, acc = native.ForwardBackward(model), native.Accs(model)
    fb.prepare(dX.ptr.value, frameOff, labOff, labs)
    cfg = native.fb_config(uFlags=uFlags, scoreMode=scoreMode)
    fb.execute(cfg, acc)
    assert (fb.results()[1] == 1).all()
    got, counts = acc.download(), fb.mix_counts()
    if two_phase:                                          # two uneven ranges of states, the last first
        acc2 = native.Accs(model)
        assert fb.execute_begin(cfg, acc2)
        fb.execute_mix(1, 3)
        fb.execute_mix(0, 1)
        fb.results()
        again = acc2.download()
        for k in KEYS + ("tr", "trOcc"):
            assert np.allclose(again[k], got[k], rtol=1e-11, atol=1e-12), k      # (equal to the order of the atomics)
    return got, counts


def oracle_accs(oracle, pk, utts, uFlags=15):
    om = oracle.Model(pk)
    oacc, ocfg = oracle.Accs(om), oracle.fb_cfg(uFlags=uFlags)
    for ut in utts:
        assert oracle.fb_utt(om, ocfg, ut["feat"], ut["seq"], oacc)[0] == 1
    return oacc


def check(got, oacc, keys=KEYS, scale="muOcc"):
    occ = np.maximum(np.asarray(getattr(oacc, scale), np.float64), 1e-3)[:, None]
    for k in keys:
        if k in ("mu", "va"):                              # sums about the current mean: the Gaussian's occupancy is an entry's scale
            ref = np.asarray(getattr(oacc, k), np.float64).reshape(occ.shape[0], -1)
            err = np.abs(np.asarray(got[k]).reshape(ref.shape) - ref)
            assert (err <= 1e-4 * np.maximum(np.abs(ref), occ)).all(), (k, float(err.max()))
        else:
            acc_close(got[k], getattr(oacc, k), k)


@pytest.mark.parametrize("D,M", [(12, 3), (45, 16), (64, 2), (65, 17), (120, 33), (128, 1)])
def test_wide_mix_against_oracle(native, oracle, D, M):
    """12: below the old sizes, even; 45: odd, a full tile; 64 / 65: the last lane of one wavefront and the first of the second, 17 a
    second tile of one component; 120 x 33: three tiles; 128: the cap, single Gaussians.  The pass counts its pairs (-1 on the list
    kernels) and defers its states, in ranges, to the same sums."""
    pk, utts = make_set(D, M)
    got, (pairs, triples) = gpu_pass(native, pk, utts, two_phase=True)
    oacc = oracle_accs(oracle, pk, utts)
    assert pairs > 0 and triples > 0
    assert float(np.max(oacc.wtOcc)) > 4 * 128            # a state's occupation is at most its pairs: its last part takes a remainder
    assert pairs % 32 != 0                                 # so some state's count is no multiple of the chunk: a ragged chunk
    check(got, oacc)


@pytest.mark.parametrize("uFlags,keys", [(1, ("mu", "muOcc")), (2, ("va", "vaOcc")), (8, ("wt", "wtOcc"))], ids=["means", "variances", "weights"])
def test_wide_mix_update_modes(native, oracle, uFlags, keys):
    """HFB.c:1697 / :1706 and the weights alone, in the exact class (the posteriors by exp())."""
    pk, utts = make_set(78, 5)
    got, counts = gpu_pass(native, pk, utts, uFlags=uFlags, scoreMode=0)
    assert min(counts) >= 0
    check(got, oracle_accs(oracle, pk, utts, uFlags=uFlags), keys, scale=keys[1])


def test_wide_mix_dead_component(native, oracle):
    pk, utts = make_set(52, 18)
    pk["compWeight"] = pk["compWeight"].copy()
    pk["compWeight"][[18 + 3, 18 + 17]] = 0.0             # one in each tile of the second state
    got, _ = gpu_pass(native, pk, utts)
    assert got["wt"][18 + 3] == 0.0 and got["wt"][18 + 17] == 0.0 and not got["mu"].reshape(-1, 52)[[18 + 3, 18 + 17]].any()
    check(got, oracle_accs(oracle, pk, utts))


def test_wide_mix_tiny_buckets(native, monkeypatch):
    """Two-pair buckets (HTKAMD_ST_CAP): nearly every pair goes through the list kernel in front of the states -- the sums of the default
    run (the list kernel takes exp() where the state kernel of the fast class takes v_exp_f32: posteriors equal to 1e-7)."""
    pk, utts = make_set(100, 20)
    whole, _ = gpu_pass(native, pk, utts)
    monkeypatch.setenv("HTKAMD_ST_CAP", "2")
    got, counts = gpu_pass(native, pk, utts)
    assert min(counts) >= 0
    for k in KEYS:
        assert np.allclose(got[k], whole[k], rtol=2e-6, atol=1e-6), k


def test_wide_mix_past_the_cap(native):
    """D = 129 keeps the list kernels: no error, nothing counted, nothing deferred."""
    from htk_amd import synth
    s = synth.generate(6, 2, 4, 2, 60, 5, D=129)
    got, counts = gpu_pass(native, s.packed(), [dict(seq=q, feat=x) for q, x in zip(s.seqs, s.feats)], scoreMode=0)
    assert counts == (-1, -1) and got["muOcc"].sum() > 0
