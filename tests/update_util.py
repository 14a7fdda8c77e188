"""Builders and a numpy restatement for the tests of the model update (tests/test_gpu_update_kernels.py).

make_set    a packed model set (the keys of SynthSet.packed()) with the shapes the launcher of htk_amd/csrc/update.hip switches on
make_stats  an accumulator vector in the layout of Accs.lay whose values are float32 numbers widened to fp64, with the edges of the
            update planted at known indices (returned beside the vector)
np_update   MLUpdateModels restated in numpy: float32 operations in the reference's order (HERest.c:795-1122, FixDiagGConst
            HModel.c:5641), every log / exp evaluated in double by the C library and rounded to float once
dispatch    the kernels the launcher picks for a set, restated from htkamd_model_update_device_begin
"""
from __future__ import annotations

import math
import os
import re

import numpy as np

F = np.float32
LZERO, MINMIX, MINLARG, TPI = -1.0e10, 1.0e-5, 2.45e-308, 6.28318530717959
UPMEANS, UPVARS, UPTRANS, UPMIXES, UPALL = 1, 2, 4, 8, 15
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the three low-count models come first: 0 examples, minEgs - 1, minEgs
LOW = 3


def cycled(ms, total):
    """ms repeated until the counts sum to `total`, the last one cut to fit"""
    out, k = [], 0
    while sum(out) < total:
        out.append(min(ms[k % len(ms)], total - sum(out))); k += 1
    return out


# id -> D, Ms, further matrices, and what the launcher must pick for it (dispatch(); the table in the test's docstring)
CASES = dict(
    a=dict(D=13, Ms=cycled([1, 2, 3, 4], 67), state="state_w<4>", gauss="fused<1>", gconst="fused", pairs=True, lastBlock=3, cutShort=True),
    b=dict(D=16, Ms=cycled([1, 2, 3, 4], 67), state="state_w<4>", gauss="fused<1>", gconst="fused", pairs=False, lastBlock=3, cutShort=False),
    c=dict(D=26, Ms=cycled([5, 16, 1, 9], 131), state="state_w<16>", gauss="fused<2>", gconst="fused", pairs=False, lastBlock=3, cutShort=True),
    d=dict(D=39, Ms=[17, 64, 2, 33, 3, 5, 2, 4, 6, 3, 2, 1, 4, 3, 5, 2, 3, 4], state="state_w<64>", gauss="fused<3>", gconst="fused", pairs=True, lastBlock=35, cutShort=True),
    e=dict(D=64, Ms=[65, 1, 3], state="trans+state", gauss="fused<4>", gconst="fused", pairs=False, lastBlock=5, cutShort=False),
    f=dict(D=49, Ms=cycled([3, 2, 4], 63), state="state_w<4>", gauss="fused<4>", gconst="fused", pairs=True, lastBlock=63, cutShort=True),
    g=dict(D=65, Ms=cycled([2, 3, 4, 5, 6], 131), state="state_w<16>", gauss="elem", gconst="lds", pairs=None, lastBlock=3, cutShort=True),
    h=dict(D=97, Ms=cycled([1, 2, 3], 129), state="state_w<4>", gauss="elem", gconst="direct", pairs=None, lastBlock=1, cutShort=True),
    i=dict(D=3, Ms=cycled([1, 2, 3, 4], 66), state="state_w<4>", gauss="fused<1>", gconst="fused", pairs=True, lastBlock=2, cutShort=True),
    j=dict(D=7, Ms=[1] * 70, state="state_w<4>", gauss="fused<1>", gconst="fused", pairs=True, lastBlock=6, cutShort=True),
    k=dict(D=13, Ms=cycled([1, 2, 3, 4], 67), tiny=253, state="state_w<4>", gauss="fused<1>", gconst="fused", pairs=True, lastBlock=3, cutShort=True),
)


def dispatch(pk):
    """What htkamd_model_update_device_begin launches for the set (update.hip, the launcher's thresholds)."""
    D, G, S, nT = int(pk["vecSize"]), int(pk["numGauss"]), int(pk["numStates"]), int(pk["numTrans"])
    maxM = int(np.diff(pk["stateCompOff"]).max())
    PS = ((2 * D + 1) + 3) & ~3
    gw = 4 if maxM <= 4 else 16 if maxM <= 16 else 64 if maxM <= 64 else 0
    out = dict(state="state_w<%d>" % gw if gw else "trans+state", nbState=(S * gw + 255) // 256 if gw else 0, nbTrans=(nT + 255) // 256)
    ldsFused = 4 * 64 * (D + PS) + 4 * 64
    if ldsFused <= 60 * 1024 and PS % 4 == 0 and D <= 64:
        out.update(gauss="fused<%d>" % min((64 * D + 1023) // 1024, 4), gconst="fused", pairs=(G * (D + 1)) % 2 == 0, lastBlock=G % 64)
    else:
        out.update(gauss="elem", gconst="lds" if 4 * 128 * D <= 48 * 1024 else "direct", pairs=None, lastBlock=G % 128)
    out["cutShort"] = (G * D) % 4 != 0
    return out


def launcher_thresholds():
    """The thresholds dispatch() restates, read from update.hip as they stand: a changed launcher fails here, not silently in the table."""
    src = open(os.path.join(ROOT, "htk_amd", "csrc", "update.hip")).read()
    return dict(
        gw=re.search(r"m->maxM <= 4 \? 4 : m->maxM <= 16 \? 16 : m->maxM <= 64 \? 64 : 0", src) is not None,
        gpb=re.search(r"#define UPD_GPB 64\b", src) is not None,
        fused=re.search(r"ldsFused <= 60 \* 1024 && \(m->PS & 3\) == 0 && m->D <= 64", src) is not None,
        nit=re.search(r"switch \(\(UPD_GPB \* m->D \+ 1023\) / 1024\)", src) is not None,
        gconst=re.search(r"const int B = 128;", src) is not None and re.search(r"sizeof\(float\) \* \(size_t\)B \* m->D > 48 \* 1024", src) is not None,
        pairs=re.search(r"\(\(a\.lay\.mu \| a\.lay\.va\) & 1\) == 0", src) is not None,
        blocks=re.search(r"\(size_t\)m->S \* gw \+ 255\) / 256", src) is not None and re.search(r"\(m->nT \+ 255\) / 256", src) is not None)


# ------------------------------------------------------------------------------------------------ the set
_LIN = [np.array([[0, 1, 0], [0, .7, .3], [0, 0, 0]]),
        # N = 5: the skip 2 -> 4 (no tee: the entry reaches state 2 only)
        np.array([[0, 1, 0, 0, 0], [0, .5, .3, .2, 0], [0, 0, .5, .5, 0], [0, 0, 0, .6, .4], [0, 0, 0, 0, 0]]),
        # N = 7: two entries, rows with two exits (2 -> 3 | 4, 4 -> 5 | 6, 5 -> 6 | 7)
        np.array([[0, .8, .2, 0, 0, 0, 0], [0, .5, .3, .2, 0, 0, 0], [0, 0, .6, .4, 0, 0, 0], [0, 0, 0, .5, .3, .2, 0],
                  [0, 0, 0, 0, .6, .2, .2], [0, 0, 0, 0, 0, .7, .3], [0, 0, 0, 0, 0, 0, 0]]),
        # N = 4: used by the model without examples only
        np.array([[0, 1, 0, 0], [0, .6, .4, 0], [0, 0, .7, .3], [0, 0, 0, 0]])]


def make_set(D, Ms, seed, tiny=0):
    """Packed set: Ms[s] components in tied state s, matrices with N = 3, 5, 7, 4 (+ `tiny` more with N = 3, one model each), models that
    share matrices and tied states, one tied state no model uses.  Models 0..2 are the ones make_stats gives 0, minEgs - 1 and minEgs
    examples; with 9 states or more their four states belong to them alone."""
    from htk_amd.synth import round_to_mmf_precision as rnd
    rng = np.random.default_rng(seed)
    S, G = len(Ms), int(sum(Ms))
    lin = list(_LIN)
    for _ in range(tiny):
        p = float(rng.uniform(0.3, 0.9))
        lin.append(np.array([[0, 1, 0], [0, p, 1 - p], [0, 0, 0]]))
    unused = S // 2 if S >= 8 else 1
    used = [s for s in range(S) if s != unused]
    if S >= 9:
        excl, pool = used[-4:], used[:-4]
    else:
        excl, pool = [used[0], used[-1], used[0], used[-1]], used
    models = [(3, excl[0:2]), (0, [excl[2]]), (0, [excl[3]])]
    i, kinds, nk = 0, (1, 2, 0), 0
    while i < len(pool):
        t = kinds[nk % 3]; nk += 1
        n = lin[t].shape[0] - 2
        st = list(pool[i:i + n]); i += n
        while len(st) < n:
            st.append(int(rng.choice(pool)))
        models.append((t, st))
    for t in (1, 2, 0):                                      # models that share tied states with the ones above
        models.append((t, [int(s) for s in rng.choice(pool, lin[t].shape[0] - 2)]))
    for k in range(tiny):
        models.append((4 + k, [int(rng.choice(pool))]))
    transN = np.array([m.shape[0] for m in lin], np.int32)
    with np.errstate(divide="ignore"):
        transP = np.concatenate([np.where(m.reshape(-1) > 0, np.log(rnd(m.reshape(-1).astype(F)).astype(np.float64)), LZERO) for m in lin]).astype(F)
    return dict(vecSize=D, numStates=S, numComp=G, numGauss=G,
                stateCompOff=np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32),
                compWeight=rnd(np.concatenate([rng.dirichlet(np.ones(m) * 4) for m in Ms]).astype(F)),
                compGauss=np.arange(G, dtype=np.int32),
                mean=rnd(rng.normal(0, 2.0, size=(G, D)).astype(F)), var=rnd(rng.uniform(0.5, 2.0, size=(G, D)).astype(F)), gconst=None,
                numTrans=len(lin), transN=transN, transOff=np.concatenate([[0], np.cumsum(transN.astype(np.int64) ** 2)]).astype(np.int32),
                transP=transP, numPhys=len(models), hmmTrans=np.array([t for t, _ in models], np.int32),
                hmmStateOff=np.concatenate([[0], np.cumsum([len(st) for _, st in models])]).astype(np.int32),
                hmmState=np.concatenate([st for _, st in models]).astype(np.int32))


def case_set(cid, seed=5):
    c = CASES[cid]
    return make_set(c["D"], c["Ms"], seed + ord(cid), tiny=c.get("tiny", 0))


def layout(pk):
    """The offsets of htkamd_accs_layout (htkamd_accs_create), as a dict"""
    G, D = int(pk["numGauss"]), int(pk["vecSize"])
    sizes = (("mu", G * D), ("muOcc", G), ("va", G * D), ("vaOcc", G), ("wt", int(pk["numComp"])), ("wtOcc", int(pk["numStates"])),
             ("tr", int(pk["transOff"][-1])), ("trOcc", int(np.sum(pk["transN"]))), ("nEgs", int(pk["numPhys"])),
             ("totalPr", 1), ("totalT", 1), ("nUttDone", 1), ("nUttSkipped", 1), ("nEval", 1))
    lay, o = {}, 0
    for name, n in sizes:
        lay[name] = o; o += n
    lay["total"] = o
    return lay


def views(pk, lay, vec):
    """the vector's sections as arrays that share its memory"""
    G, D = int(pk["numGauss"]), int(pk["vecSize"])
    sec = lambda a, b: vec[lay[a]:lay[b]]
    return dict(mu=sec("mu", "muOcc").reshape(G, D), muOcc=sec("muOcc", "va"), va=sec("va", "vaOcc").reshape(G, D), vaOcc=sec("vaOcc", "wt"),
                wt=sec("wt", "wtOcc"), wtOcc=sec("wtOcc", "tr"), tr=sec("tr", "trOcc"), trOcc=sec("trOcc", "nEgs"), nEgs=sec("nEgs", "totalPr"))


def model_states(pk, h):
    return [int(s) for s in pk["hmmState"][pk["hmmStateOff"][h]:pk["hmmStateOff"][h + 1]]]


# ------------------------------------------------------------------------------------------------ the statistics
def make_stats(pk, lay, seed, plant=True, minEgs=1, floors=None, mixFloor=6e-5, above=False):
    """(vec, planted).  Base: occupancies U(0.5, 50), mu = occ d, va = occ (v' + d^2), weights that sum to wtOcc, transition rows that sum
    to trOcc -- all float32 numbers.  plant: the edges below, each at the index `planted` names.  floors [D]: the variance floor the
    update will run with (minVar as a constant vector, or the varFloor vector); None: minVar = 0, and the planted variances are the ones
    that cancel to 0 / come out negative.  above: two ratios above 1.001 (the update must refuse: a case of its own)."""
    rng = np.random.default_rng(seed)
    G, D, S, H = int(pk["numGauss"]), int(pk["vecSize"]), int(pk["numStates"]), int(pk["numPhys"])
    off, Ms = pk["stateCompOff"], np.diff(pk["stateCompOff"])
    vec = np.zeros(lay["total"], np.float64)
    v = views(pk, lay, vec)
    occ = rng.uniform(0.5, 50, G).astype(F)
    d = rng.normal(0, 0.3, (G, D)).astype(F)
    v["muOcc"][:] = occ; v["vaOcc"][:] = occ
    v["mu"][:] = occ[:, None] * d
    vp = rng.uniform(0.5, 2.0, (G, D)).astype(F)
    v["va"][:] = occ[:, None] * (vp + d * d)
    for s in range(S):
        o = F(rng.uniform(1, 100))
        v["wtOcc"][s] = o
        v["wt"][off[s]:off[s + 1]] = (o * rng.dirichlet(np.ones(Ms[s]) * 4).astype(F)) if Ms[s] > 1 else o
    occOff = np.concatenate([[0], np.cumsum(pk["transN"])])
    for t in range(int(pk["numTrans"])):
        N = int(pk["transN"][t])
        P = pk["transP"][pk["transOff"][t]:pk["transOff"][t + 1]].reshape(N, N)
        for i in range(N - 1):
            live = np.nonzero(P[i] > -0.5e10)[0]
            o = F(rng.uniform(1, 50))
            v["trOcc"][occOff[t] + i] = o
            v["tr"][pk["transOff"][t] + i * N + live] = o * rng.dirichlet(np.ones(len(live)) * 3).astype(F)
    n = rng.integers(minEgs + 1, 20, H).astype(np.float64)
    planted = dict(expect={})
    if not plant:
        v["nEgs"][:] = n
        return vec, planted
    # ---- example counts: 0, minEgs - 1, minEgs; every fifth one-matrix model without examples
    n[0], n[1], n[2] = 0, max(minEgs - 1, 0), minEgs
    tinyDead = [h for h in range(H) if pk["hmmTrans"][h] >= 4 and (int(pk["hmmTrans"][h]) % 5 == 0 or pk["hmmTrans"][h] == pk["numTrans"] - 1)]
    n[tinyDead[:-1]] = 0                                      # (the last matrix keeps its model: its row without occupancy is counted)
    v["nEgs"][:] = n
    qual = [h for h in range(H) if n[h] >= minEgs and n[h] > 0]
    qualS = sorted({s for h in qual for s in model_states(pk, h)})
    usedS = sorted({int(s) for s in pk["hmmState"]})
    sure = sorted({s for h in range(LOW, H) if h in qual for s in model_states(pk, h)})       # qualify whatever minEgs is
    planted.update(nEgs=n.astype(int), qualModels=qual, qualStates=qualS, unusedStates=[s for s in range(S) if s not in usedS],
                   deadTrans=[int(pk["hmmTrans"][h]) for h in tinyDead[:-1]] + ([3] if 3 not in {int(pk["hmmTrans"][h]) for h in qual} else []),
                   nonqualGauss=[g for s in usedS if s not in qualS for g in range(off[s], off[s + 1])],
                   atMinEgsGauss=[g for s in model_states(pk, 2) if s not in sure for g in range(off[s], off[s + 1])])
    planted["expect"]["nSkippedHmm"] = int((n < minEgs).sum())
    # ---- weights.  The states are taken from the ones that qualify under every minEgs, largest mixtures first
    free = sorted(sure, key=lambda s: (-Ms[s], s))
    take = lambda minM: next((free.pop(k) for k in range(len(free)) if Ms[free[k]] >= minM), None)
    maxM = int(Ms.max())
    if maxM > 1:
        sA = take(3)
        if sA is not None:                                    # below MINMIX, exactly 0, (M >= 4) between MINMIX and the mixture floor
            c0, o = off[sA], v["wtOcc"][sA]
            v["wt"][c0] = F(o * F(5e-6)); v["wt"][c0 + 1] = 0.0
            planted.update(belowMinMix=int(c0), zeroWeight=int(c0 + 1), stateDead=int(sA))
            if Ms[sA] >= 4:
                v["wt"][c0 + 2] = F(o * F(3e-5)); planted["belowFloor"] = [int(c0 + 2)]
        sB = take(2)
        if sB is not None:                                    # a ratio in (1, 1.001]: clipped to 1, no error
            c0, o = off[sB], F(v["wtOcc"][sB])
            v["wt"][c0] = F(o * F(1.0005)); v["wt"][c0 + 1:off[sB + 1]] = F(o * F(1e-3))
            assert 1.0 < float(F(v["wt"][c0]) / o) <= 1.001
            planted.update(ratioAboveOne=int(c0), stateClip=int(sB))
            if above:
                v["wt"][c0:c0 + 2] = F(o * F(1.01)); planted["expect"]["nWeightAboveOne"] = 2
        sC = take(1)
        if sC is not None:
            v["wtOcc"][sC] = 0.0; planted["stateNoOcc"] = int(sC); planted["expect"]["nNoMixUse"] = 1
        # (a mixture narrower than the lane group of k_upd_state_w where there is one: lanes past M take part in its __shfl loop)
        sD = next((free.pop(k) for k in range(len(free)) if Ms[free[k]] >= 2 and Ms[free[k]] not in (4, 16, 64)), None) or take(2)
        if sD is not None:                                    # FloorMixes: one weight below the floor (above MINMIX) ...
            v["wt"][off[sD]] = F(v["wtOcc"][sD] * F(0.5 * mixFloor)); planted.setdefault("belowFloor", []).append(int(off[sD])); planted["stateSomeBelow"] = int(sD)
        sF = take(2)
        if sF is not None:                                    # ... all of them below it (sum == 0: no rescale) ...
            v["wt"][off[sF]:off[sF + 1]] = F(v["wtOcc"][sF] * F(0.3 * mixFloor)); planted["stateAllBelow"] = int(sF)
        sE = take(2)                                          # ... none below it (fsum == 0): left as drawn
        if sE is not None:
            planted["stateNoneBelow"] = int(sE)
    planted["expect"].setdefault("nNoMixUse", 0)
    # ---- Gaussians: from the states not planted above, else the live components of the first planted one
    cand = [g for s in free for g in range(off[s], off[s + 1])]
    if len(cand) < 3:
        cand = list(range(off[planted["stateDead"]] + 3, off[planted["stateDead"] + 1]))
    g1, g2, g3 = [int(g) for g in rng.choice(cand, 3, replace=False)]
    v["vaOcc"][g1] = 0.0                                      # no variance statistics: variance kept, mean moved, counted
    v["muOcc"][g2] = 0.0                                      # no mean statistics: mean kept, variance without the mean-shift term
    v["muOcc"][g3] = v["vaOcc"][g3] = 8.0                     # x = va / 8 - (mu / 8)^2 without a rounding
    v["mu"][g3] = F(8) * d[g3]; v["va"][g3] = F(8) * (vp[g3] + d[g3] * d[g3])
    planted.update(noVarOcc=g1, noMuOcc=g2, varGauss=g3)
    planted["expect"]["nNoVarUse"] = 1
    if floors is None:
        v["mu"][g3, 0:3] = (4.0, 4.0, 0.0); v["va"][g3, 0:3] = (2.0, 1.0, 0.0)       # cancels to 0; negative; 0 without a mean
        planted.update(varZero=[(g3, 0), (g3, 1), (g3, 2)], varFloored=[(g3, 1)])
    else:
        fl = np.asarray(floors, F)
        v["mu"][g3, 0:3] = 0.0
        v["va"][g3, 0:3] = (F(8) * F(fl[0] * F(0.5)), F(8) * fl[1], F(8) * np.nextafter(fl[2], F(np.inf)))
        planted.update(varBelow=(g3, 0), varOnFloor=(g3, 1), varUlpAbove=(g3, 2))
    # ---- transitions: a row without occupancy (N = 7, row 3), a transition that underflows to 0 (N = 5, the skip 2 -> 4)
    v["trOcc"][occOff[2] + 2] = 0.0
    v["tr"][pk["transOff"][1] + 1 * 5 + 3] = float(np.nextafter(F(0), F(1)))
    planted.update(rowNoOcc=(2, 3), transUnderflow=int(pk["transOff"][1] + 1 * 5 + 3))
    planted["expect"]["nNoTransOut"] = 1
    if pk["numTrans"] > 4:
        t = int(pk["numTrans"]) - 1
        v["trOcc"][occOff[t] + 1] = 0.0; planted["expect"]["nNoTransOut"] += 1
    assert np.array_equal(vec, vec.astype(F).astype(np.float64))
    return vec, planted


# ------------------------------------------------------------------------------------------------ the restatement
def _logf(x):
    return F(math.log(float(x)))


def mix_log_weight(w):
    return F(LZERO) if float(w) < MINMIX else _logf(w)


def _round_trip_var(x):
    x = np.minimum(x, F(1e30)); x = np.maximum(x, F(1e-30))
    iv = F(1) / x
    iv = np.minimum(iv, F(1e30)); iv = np.maximum(iv, F(1e-30))
    return F(1) / iv


def fix_gconst(var):
    s = F(len(var) * math.log(TPI))
    for x in var:
        s = F(s + (F(LZERO) if float(x) <= MINLARG else _logf(x)))
    return s


def start_params(pk):
    G, D = int(pk["numGauss"]), int(pk["vecSize"])
    var = np.array(pk["var"], F).reshape(G, D)
    gconst = np.array([fix_gconst(var[g]) for g in range(G)], F) if pk.get("gconst") is None else np.array(pk["gconst"], F)
    return dict(mean=np.array(pk["mean"], F).reshape(G, D), var=var, gconst=gconst, compWeight=np.array(pk["compWeight"], F), transP=np.array(pk["transP"], F))


def np_update(pk, lay, vec, minEgs=3, minVar=0.0, mixWeightFloor=0.0, uFlags=UPALL, singleProcess=False, varFloor=None, rowNormalise=False):
    """(parameters, prepared tables, counters) after MLUpdateModels on the set `pk` from the accumulator vector."""
    G, D, S, H = int(pk["numGauss"]), int(pk["vecSize"]), int(pk["numStates"]), int(pk["numPhys"])
    off = pk["stateCompOff"]
    maxM = int(np.diff(off).max())
    a = {k: x.astype(F) for k, x in views(pk, lay, np.array(vec, np.float64)).items()}       # every sum rounded to float once
    p = start_params(pk)
    mean, var, gconst, w, tp = p["mean"], p["var"], p["gconst"], p["compWeight"], p["transP"]
    st = dict(nFloorVar=0, nFloorVarMix=0, nSkippedHmm=0, nNoTransOut=0, nNoMixUse=0, nNoVarUse=0, nWeightAboveOne=0, nMapObserved=0)
    floor = F(mixWeightFloor)
    fl = np.asarray(varFloor, F) if varFloor is not None else np.full(D, F(minVar), F)
    if singleProcess:                                          # ConvDiagC / ConvLogWt before the pass, ForceDiagC / ConvExpWt after it
        for s in sorted({int(s) for s in pk["hmmState"]}):
            for c in range(off[s], off[s + 1]):
                var[c] = _round_trip_var(var[c])
                w[c] = F(math.exp(float(mix_log_weight(w[c]))))
    nEgs = [int(round(x)) for x in views(pk, lay, np.array(vec, np.float64))["nEgs"]]
    st["nSkippedHmm"] = sum(n < minEgs for n in nEgs)
    qual = [h for h in range(H) if nEgs[h] >= minEgs and nEgs[h] > 0]
    occOff = np.concatenate([[0], np.cumsum(pk["transN"])])
    if uFlags & UPTRANS:                                       # UpdateTrans; rowNormalise: HRest's RestTransP
        for t in sorted({int(pk["hmmTrans"][h]) for h in qual}):
            N, o = int(pk["transN"][t]), int(pk["transOff"][t])
            for i in range(N - 1):
                occi = a["trOcc"][occOff[t] + i]
                if not occi > 0:
                    st["nNoTransOut"] += 1
                    continue
                x = a["tr"][o + i * N + 1:o + i * N + N] / occi
                if rowNormalise:
                    tot = F(0)
                    for xj in x:
                        tot = F(tot + xj)
                    x = x / tot
                    tp[o + i * N + 1:o + i * N + N] = [F(LZERO) if float(xj) < MINLARG else _logf(xj) for xj in x]
                else:
                    tp[o + i * N + 1:o + i * N + N] = [_logf(xj) if float(xj) > MINLARG else F(LZERO) for xj in x]
    qualS = sorted({s for h in qual for s in model_states(pk, h)})
    if maxM > 1 and (uFlags & UPMIXES):                        # UpdateWeights + FloorMixes
        for s in qualS:
            occi = a["wtOcc"][s]
            if not occi > 0:
                st["nNoMixUse"] += 1
                continue
            x = a["wt"][off[s]:off[s + 1]] / occi
            st["nWeightAboveOne"] += int((x.astype(np.float64) > 1.001).sum())
            x = np.minimum(x, F(1))
            x = np.where(x.astype(np.float64) > MINMIX, x, F(0)).astype(F)
            if floor > 0:
                tot, ftot = F(0), F(0)
                for k in range(len(x)):
                    if x[k] > floor:
                        tot = F(tot + x[k])
                    else:
                        ftot = F(ftot + floor); x[k] = floor
                if ftot != 0 and tot != 0:
                    scale = F((1.0 - float(ftot)) / float(tot))
                    x = np.where(x > floor, x * scale, x).astype(F)
            w[off[s]:off[s + 1]] = x
    for s in qualS:                                            # the Gaussians of the live components of the marked states
        for c in range(off[s], off[s + 1]):
            if not float(w[c]) > MINMIX:
                continue
            g = int(pk["compGauss"][c])
            muOcc, vaOcc = a["muOcc"][g], a["vaOcc"][g]
            if uFlags & UPVARS:                                # UpdateVars: before the means, from the OLD mean's statistics
                if vaOcc > 0:
                    shift = (uFlags & UPMEANS) and muOcc > 0
                    muDiff = a["mu"][g] / muOcc if shift else np.zeros(D, F)
                    x = a["va"][g] / vaOcc - muDiff * muDiff
                    low = x < fl
                    st["nFloorVar"] += int(low.sum()); st["nFloorVarMix"] += int(low.any())
                    var[g] = np.where(low, fl, x)
                else:
                    st["nNoVarUse"] += 1
            if (uFlags & UPMEANS) and muOcc > 0:               # UpdateMeans
                mean[g] = mean[g] + a["mu"][g] / muOcc
            if uFlags & (UPMEANS | UPVARS):
                gconst[g] = fix_gconst(var[g])
    assert all(x.dtype == F for x in (mean, var, gconst, w, tp))
    prepared = dict(ivar=F(1) / np.maximum(np.minimum(var, F(1e30)), F(1e-30)), gconst=gconst.copy(), compLogWt=np.array([mix_log_weight(x) for x in w], F))
    return p, prepared, st


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_update(oracle, pk, lay, vec, **kw):
    """oracle.update (orc_update) from the same float32 values: (parameters, prepared, its three counters)"""
    om = oracle.Model(pk)
    oa = oracle.Accs(om)
    v = views(pk, lay, np.array(vec, np.float64))
    for k in ("mu", "muOcc", "va", "vaOcc", "wt", "wtOcc", "tr", "trOcc"):
        getattr(oa, k)[...] = v[k].astype(F).reshape(getattr(oa, k).shape)
    oa.nEgs[:] = np.round(v["nEgs"]).astype(np.int32)
    st = oracle.update(om, oa, **kw)
    return (dict(mean=om.mean, var=om.var, gconst=om.gconst, compWeight=om.compWeight, transP=om.transP),
            dict(ivar=om.ivar, gconst=om.gconst, compLogWt=om.compLogWt), st)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, F).reshape(-1), np.ascontiguousarray(y, F).reshape(-1)
    return x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
