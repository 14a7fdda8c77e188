#!/usr/bin/env python3
"""The two tiny model sets of tests/test_gpu_model_tables.py with their HTKAMD_SCORE_MFMA scores, written to
tests/golden/model_tables/{W,N}.npz.  Needs a GPU.

The scores were recorded on commit 25a95e1 ("Input transforms: <INPUTXFORM> / ~j sets, applied on the device"), the last one whose
fp32 fragment table was built by a host loop at creation (mfma_refresh, csrc/model.hip); the test asks the device builder
(k_upd_mfma, csrc/update.hip) for the same bits.  Running the script on a later commit records that commit's scores instead.

    W   D = 39 ("wide" kernels, the dense five-k-step bf16 layout): four states of 1, 3, 16 and 16 components, the second component of
        the 3-component state with a weight below MINMIX (a dead column)
    N   D = 10 (general kernels; 5 k-steps padded to 7): three states of 1, 17 and 5 components -- the 17-component state takes two
        tiles, the second with 15 empty columns

Every state is the one emitting state of a 3-state model of its own.  Each file holds the packed description, 40 frames X, the
scores [40, states] of a freshly created model, and an accumulator's worth of statistics for the updates (occupations, first and
second moments about the means), so that no random generator has to reproduce any of it.

    python tests/golden/make_model_tables_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "model_tables")
T = 40


def make_set(D, nmix, dead, seed):
    rng = np.random.default_rng(seed)
    S, G = len(nmix), sum(nmix)
    off = np.concatenate([[0], np.cumsum(nmix)]).astype(np.int32)
    w = np.concatenate([rng.dirichlet(np.ones(m) * 4) for m in nmix])
    if dead is not None:                                   # a weight below MINMIX = 1e-5, the state's other weights scaled to sum 1
        s, j = dead
        c = off[s] + j
        w[off[s]:off[s + 1]] *= (1.0 - 1.0e-6) / (1.0 - w[c]); w[c] = 1.0e-6
    mean = rng.normal(0, 1.0, size=(G, D)).astype(np.float32)
    var = rng.uniform(0.5, 2.0, size=(G, D)).astype(np.float32)
    with np.errstate(divide="ignore"):
        tp = np.array([[0, 1, 0], [0, .8, .2], [0, 0, 0]])
        transP = np.where(tp > 0, np.log(tp), -1.0e10).astype(np.float32).reshape(-1)
    pk = dict(vecSize=D, numStates=S, numComp=G, numGauss=G, stateCompOff=off, compWeight=w.astype(np.float32),
              compGauss=np.arange(G, dtype=np.int32), mean=mean, var=var, numTrans=1, transN=np.array([3], np.int32),
              transOff=np.array([0, 9], np.int32), transP=transP, numPhys=S, hmmTrans=np.zeros(S, np.int32),
              hmmStateOff=np.arange(S + 1, dtype=np.int32), hmmState=np.arange(S, dtype=np.int32))
    comp = rng.integers(0, G, size=T)
    X = (mean[comp] + rng.normal(0, 1, size=(T, D)) * np.sqrt(var[comp])).astype(np.float32)
    # statistics as a pass leaves them (HFB.c UpMixParms): occupation, sum of occ * (x - mean), sum of occ * (x - mean)^2
    occ = rng.uniform(5.0, 20.0, size=G)
    if dead is not None:
        occ[off[dead[0]] + dead[1]] = 0.0
    shift = rng.normal(0, 0.2, size=(G, D))
    spread = var * rng.uniform(0.7, 1.3, size=(G, D))
    stats = dict(occ=occ, mu=occ[:, None] * shift, va=occ[:, None] * (spread + shift * shift))
    return pk, X, stats


SETS = dict(W=dict(D=39, nmix=[1, 3, 16, 16], dead=(1, 1), seed=3901), N=dict(D=10, nmix=[1, 17, 5], dead=None, seed=1001))


def main():
    from htk_amd import capi
    os.makedirs(OUT, exist_ok=True)
    for name, kw in SETS.items():
        pk, X, stats = make_set(**kw)
        m = capi.Model(dict(pk, gconst=None))
        mfma = m.outp_block(X, np.arange(pk["numStates"], dtype=np.int32), capi.SCORE_MFMA)
        m.close()
        np.savez_compressed(os.path.join(OUT, name + ".npz"), X=X, mfma=mfma, **pk, **{"stat_" + k: v for k, v in stats.items()})
        print(name, "scores", mfma.shape, "min", mfma.min(), "max", mfma.max())


if __name__ == "__main__":
    main()
