"""Full-covariance (FULLC) scoring on the device: the exact kernel (gmm_full.hip) against the reference's FOutP scores and against a NumPy
restatement of FOutP with the reference's operation order, in both mixture forms; the matrix-core score modes and re-estimation are
refused for such a model.  Fixtures: tests/golden/make_fullc_golden.py."""
import importlib.util
import math
import os
import subprocess

import numpy as np
import pytest

from htk_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FC = os.path.join(GOLD, "fullc")
LST = os.path.join(GOLD, "demo", "bcplist")
LZERO, LSMALL, LMINMIX = -1.0e10, -0.5e10, -11.5129254649702
MINLOGEXP = -math.log(-LZERO)
_spec = importlib.util.spec_from_file_location("make_fullc_golden", os.path.join(GOLD, "make_fullc_golden.py"))
mfg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mfg)            # (the fixture recipe's HVite switches; the script does nothing on import)


def ladd(x, y):
    """LAdd (HMath.c) in double."""
    if x < y:
        x, y = y, x
    diff = y - x
    if diff < MINLOGEXP:
        return LZERO if x < LSMALL else x
    return x + math.log(1.0 + math.exp(diff))


def fout_p(X, mean, tri):
    """FOutP over the rows of X, float32, the reference's order: off-diagonal sum, *2, + gConst, diagonal terms, -0.5 in double."""
    D = X.shape[1]
    xmm = (X - mean).astype(np.float32)
    s = np.zeros(X.shape[0], np.float32)
    for j in range(D - 1):
        for i in range(j + 1, D):
            s = s + (xmm[:, i] * xmm[:, j]) * tri[i * (i + 1) // 2 + j]
    return s, xmm


def fout_p_close(s, xmm, tri, gconst):
    D = xmm.shape[1]
    s = s * np.float32(2.0)
    s = s + np.float32(gconst)
    for i in range(D):
        s = s + (xmm[:, i] * xmm[:, i]) * tri[i * (i + 1) // 2 + i]
    return (-0.5 * s.astype(np.float64)).astype(np.float32)


def ref_scores(pk, logwt, X, states, soutp):
    D = X.shape[1]
    G = pk["mean"].shape[0]
    px = np.empty((G, X.shape[0]), np.float32)
    for g in range(G):
        s, xmm = fout_p(X, pk["mean"][g], pk["invCov"][g])
        px[g] = fout_p_close(s, xmm, pk["invCov"][g], pk["gconst"][g])
    out = np.empty((X.shape[0], len(states)), np.float32)
    off = pk["stateCompOff"]
    for k, st in enumerate(states):
        c0, c1 = off[st], off[st + 1]
        if c1 - c0 == 1:
            out[:, k] = px[pk["compGauss"][c0]]
            continue
        for t in range(X.shape[0]):
            if soutp:
                acc = LZERO
                for c in range(c0, c1):
                    if logwt[c] > np.float32(LMINMIX):
                        acc = ladd(acc, float(logwt[c]) + float(px[pk["compGauss"][c], t]))
                out[t, k] = np.float32(acc)
            else:
                acc = np.float32(LZERO)
                for c in range(c0, c1):
                    if logwt[c] > np.float32(LMINMIX):
                        acc = np.float32(ladd(float(acc), float(np.float32(logwt[c] + px[pk["compGauss"][c], t]))))
                out[t, k] = acc
    return out


def random_fullc(D, NS, M, seed):
    """A synthetic set with random positive-definite inverse covariances (correlated, condition number ~ 10-100)."""
    s = synth.generate(NS=NS, M=M, NP=max(NS // 3, 1), NU=2, T=90, seed=seed, D=D, write_data=False)
    pk = s.packed()
    rng = np.random.default_rng(seed)
    G = pk["mean"].shape[0]
    tri = np.empty((G, D * (D + 1) // 2), np.float32)
    for g in range(G):
        A = rng.normal(0, 1, (D, D)) / math.sqrt(D)
        P = A @ A.T + np.diag(rng.uniform(0.3, 1.5, D))
        tri[g] = P[np.tril_indices(D)].astype(np.float32)      # row-major lower triangle: (i, j), j <= i
    pk["invCov"] = tri
    pk["gconst"] = None
    X = np.concatenate(s.feats).astype(np.float32)
    assert X.shape[1] == D
    return pk, X


def test_soutp_scores_equal_the_reference(native):
    native.check(native.lib().htkamd_set_device(0), "set_device")
    mmf = native.Mmf(files=[os.path.join(FC, "fullc_in")], hmm_list=LST)
    pk = mmf.packed()
    m = native.Model(pk)
    stat, _, _ = native.parm_read(os.path.join(GOLD, "demo", "train", "tr1.mfc"))
    dX, _, cols = native.parm_add_qualifiers([stat], hasD=True)                      # TARGETKIND = MFCC_E_D, as ref_outp reads it
    X = dX.to_host(np.float32, (stat.shape[0], cols))
    assert cols == pk["vecSize"] == 26
    H = pk["numPhys"]
    ref = np.fromfile(os.path.join(FC, "outp_tr1.bin"), np.float32).reshape(X.shape[0], H, -1)
    off = pk["hmmStateOff"]
    phys = [mmf.logical[n] for n in open(LST).read().split()]                       # ref_outp's columns follow the HMM list
    states = np.concatenate([pk["hmmState"][off[h]:off[h + 1]] for h in phys]).astype(np.int32)
    want = np.concatenate([ref[:, k, :off[h + 1] - off[h]] for k, h in enumerate(phys)], axis=1)
    got = m.outp_block(X, states, mode=native.SCORE_SOUTP)
    assert np.array_equal(got, want), np.abs(got - want).max()
    got2 = m.outp_block(X, states)                                   # ShStrP's form: single Gaussians, the same numbers
    assert np.array_equal(got2, want)


@pytest.mark.parametrize("D,M", [(39, 3), (13, 4), (39, 1), (7, 2)])
def test_synthetic_sets_equal_a_restatement_of_foutp(native, D, M):
    native.check(native.lib().htkamd_set_device(0), "set_device")
    pk, X = random_fullc(D, NS=6, M=M, seed=100 + D + M)
    m = native.Model(pk)
    prm = m.get_params()
    pk["gconst"] = prm["gconst"]                          # FixFullGConst at creation: finite, and what the kernel reads
    assert np.isfinite(prm["gconst"]).all() and np.array_equal(prm["invCov"], pk["invCov"])
    logwt = m.get_prepared()["compLogWt"]
    states = np.arange(pk["numStates"], dtype=np.int32)
    X = X[:150]
    for soutp in (False, True):
        got = m.outp_block(X, states, mode=native.SCORE_SOUTP if soutp else native.SCORE_EXACT)
        want = ref_scores(pk, logwt, X, states, soutp)
        assert np.array_equal(got, want), (D, M, soutp, np.abs(got - want).max())


def test_set_inv_cov_writes_through(native):
    native.check(native.lib().htkamd_set_device(0), "set_device")
    pk, X = random_fullc(13, NS=3, M=2, seed=7)
    m = native.Model(pk)
    states = np.arange(pk["numStates"], dtype=np.int32)
    before = m.outp_block(X[:40], states)
    tri = pk["invCov"] * np.float32(2.0)
    m.set_inv_cov(tri)
    prm = m.get_params()
    assert np.array_equal(prm["invCov"], tri)
    pk2 = dict(pk, invCov=tri, gconst=prm["gconst"])
    want = ref_scores(pk2, m.get_prepared()["compLogWt"], X[:40], states, False)
    after = m.outp_block(X[:40], states)
    assert np.array_equal(after, want) and not np.array_equal(after, before)
    bad = tri.copy(); bad[0, 0] = -1.0
    with pytest.raises(native.HtkAmdError):
        m.set_inv_cov(bad)


def test_what_a_fullc_model_refuses(native):
    native.check(native.lib().htkamd_set_device(0), "set_device")
    pk, X = random_fullc(13, NS=3, M=2, seed=9)
    m = native.Model(pk)
    states = np.arange(pk["numStates"], dtype=np.int32)
    for mode in (native.SCORE_MFMA, native.SCORE_BF16, native.SCORE_F16, native.SCORE_DIAGC):
        with pytest.raises(native.HtkAmdError):
            m.outp_block(X[:20], states, mode=mode)
    with pytest.raises(native.HtkAmdError):
        native.ForwardBackward(m)
    with pytest.raises(native.HtkAmdError):
        native.Accs(m)
    with pytest.raises(native.HtkAmdError):
        m.set_params(var=np.ones((m.G, m.D), np.float32))
    assert native.lib().htkamd_model_is_full(m.h) == 1


def _cli(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def test_cli_tools_on_a_fullc_set(native, tmp_path):
    """tools/bin/hvite recognises and aligns with fullc_in as the reference's HVite does, byte for byte (the same switches:
    make_fullc_golden.RECOGNISE / ALIGN); a non-exact score mode is refused by name; tools/bin/herest refuses to re-estimate the set
    instead of running a DIAGC pass over it."""
    from htk_amd import build as nbuild
    nbuild.build_tools()
    hvite, herest = os.path.join(ROOT, "tools", "bin", "hvite"), os.path.join(ROOT, "tools", "bin", "herest")
    conf = tmp_path / "c"; conf.write_text("TARGETKIND = MFCC_E_D\n")
    demo = os.path.join(GOLD, "demo")
    train = sorted(os.path.join(demo, "train", f) for f in os.listdir(os.path.join(demo, "train")) if f.endswith(".mfc"))
    test = sorted(os.path.join(demo, "test", f) for f in os.listdir(os.path.join(demo, "test")) if f.endswith(".mfc"))
    base = [hvite, "-C", str(conf), "-H", os.path.join(FC, "fullc_in")]
    for sub, opts, files in (("rec_test", mfg.RECOGNISE, test), ("rec_align", mfg.ALIGN, train[:2])):
        out = tmp_path / sub; out.mkdir()
        r = _cli(base + ["-l", str(out)] + opts + [os.path.join(demo, "bcpvocab"), LST] + files)
        assert r.returncode == 0, r.stderr
        want = sorted(os.listdir(os.path.join(FC, sub)))
        assert sorted(os.listdir(str(out))) == want and len(want) == len(files)
        for f in want:
            assert (out / f).read_bytes() == open(os.path.join(FC, sub, f), "rb").read(), (sub, f)
    r = _cli(base + ["--score", "fast", "-l", str(tmp_path)] + mfg.RECOGNISE + [os.path.join(demo, "bcpvocab"), LST] + test[:1])
    assert r.returncode != 0 and "FULLC" in r.stderr and "exact" in r.stderr, r.stderr
    r = _cli([herest, "-C", str(conf), "-H", os.path.join(FC, "fullc_in"), "-L", os.path.join(demo, "labels"), "-M", str(tmp_path), LST] + train)
    assert r.returncode != 0 and "FULLC" in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "fullc_in"))
