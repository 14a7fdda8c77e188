"""htkamd_model_update_device (htk_amd/csrc/update.hip), every kernel path, from planted statistics.

The update needs no forward-backward pass: Accs.upload_add takes any vector in Accs.lay's layout.  tests/update_util.py builds small sets
with the shapes the launcher switches on and statistics with the update's edges at known indices; the references are the host C update
(Model.update), the oracle's orc_update where it applies (no varFloor vector, no rowNormalise) and a numpy restatement -- the three agree
bit for bit, and the device must match the host as section "what the device must match" below states."""
import functools
import re

import numpy as np
import pytest

import update_util as uu
from update_util import F, LZERO, UPMEANS, UPVARS, UPTRANS, UPMIXES, UPALL

gpu = pytest.mark.gpu
MIXFLOOR = 2e-5 * 3


def _vfloor(D):
    return np.linspace(0.4, 1.2, D).astype(F)


# name -> (keywords of the update, the oracle applies)
CONFIGS = dict(
    plain=(dict(minEgs=1), True),
    single=(dict(minEgs=1, singleProcess=True), True),
    minvar=(dict(minEgs=1, minVar=0.7, mixWeightFloor=MIXFLOOR), True),
    floors=(dict(minEgs=1, minVar=0.7, mixWeightFloor=MIXFLOOR, varFloor=_vfloor), False),
    flags_mt=(dict(minEgs=1, uFlags=UPMEANS | UPTRANS, singleProcess=True), True),
    flags_v=(dict(minEgs=1, uFlags=UPVARS), True),
    minegs3=(dict(minEgs=3), True),
    minegs0=(dict(minEgs=0), True),
    rownorm=(dict(minEgs=1, rowNormalise=True), False),
)
CASE_IDS = sorted(uu.CASES)


def _kw(cfg, D):
    kw = dict(CONFIGS[cfg][0])
    if "varFloor" in kw:
        kw["varFloor"] = kw["varFloor"](D)
    return kw


def _floors(kw, D):
    if kw.get("varFloor") is not None:
        return np.asarray(kw["varFloor"], F)
    return np.full(D, F(kw["minVar"]), F) if kw.get("minVar", 0.0) > 0 else None


@functools.lru_cache(maxsize=None)
def _set(cid):
    return uu.case_set(cid)


@functools.lru_cache(maxsize=None)
def _stats(cid, cfg, seed=3, above=False):
    pk = _set(cid)
    kw = _kw(cfg, int(pk["vecSize"]))
    vec, planted = uu.make_stats(pk, uu.layout(pk), seed, minEgs=kw["minEgs"], floors=_floors(kw, int(pk["vecSize"])), mixFloor=MIXFLOOR, above=above)
    vec.setflags(write=False)
    return vec, planted


@functools.lru_cache(maxsize=None)
def _restated(cid, cfg):
    pk = _set(cid)
    return uu.np_update(pk, uu.layout(pk), _stats(cid, cfg)[0], **_kw(cfg, int(pk["vecSize"])))


# ------------------------------------------------------------------------------------------------ without a device
def test_case_table_matches_the_launcher():
    """Every row of the case table takes the path it is there for, by the launcher's thresholds as update.hip has them."""
    th = uu.launcher_thresholds()
    assert all(th.values()), "the launcher's thresholds changed: restate them in update_util.dispatch and the case table (%s)" % th
    for cid, c in uu.CASES.items():
        pk = _set(cid)
        d = uu.dispatch(pk)
        for k in ("state", "gauss", "gconst", "pairs", "lastBlock", "cutShort"):
            assert d[k] == c[k], (cid, k, d[k], c[k])
        Ms = np.diff(pk["stateCompOff"])
        assert int(pk["numGauss"]) == sum(c["Ms"]) <= 300 and (len(set(Ms)) > 1 or cid == "j") and len(set(pk["transN"][:3])) == 3
        assert len(set(int(s) for s in pk["hmmState"])) == int(pk["numStates"]) - 1         # one tied state no model uses
    assert uu.CASES["a"]["Ms"][:4] == [1, 2, 3, 4] and (67 * 13) % 4 == 3
    k = uu.dispatch(_set("k"))
    assert int(_set("k")["numTrans"]) == 257 and k["nbTrans"] == 2 and k["nbState"] == 1 and (int(_set("k")["numStates"]) * 4) % 256 != 0
    assert uu.dispatch(_set("c"))["lastBlock"] == 3 and int(_set("c")["numGauss"]) == 131
    assert int(_set("g")["numGauss"]) * 65 % 4 == 3 and int(_set("h")["numGauss"]) == 129 and int(_set("f")["numGauss"]) == 63
    assert int(_set("d")["numGauss"]) % 2 == 1 and int(_set("d")["numGauss"]) >= 129
    assert (64 * 3) % 4 == 0 and 3 % 4 != 0                                                  # (i): a 16-byte word spans Gaussians


def test_every_edge_is_planted():
    """The sets with room for it carry every edge; the small ones (e: two states in use, j: no mixtures) what fits."""
    everything = {"belowMinMix", "zeroWeight", "belowFloor", "ratioAboveOne", "stateNoOcc", "stateSomeBelow", "stateAllBelow", "stateNoneBelow",
                  "noVarOcc", "noMuOcc", "varZero", "rowNoOcc", "transUnderflow", "nonqualGauss", "unusedStates"}
    for cid in CASE_IDS:
        pl = _stats(cid, "plain")[1]
        have = {k for k in everything if pl.get(k) not in (None, [])}
        if cid == "j":
            assert have >= {"noVarOcc", "noMuOcc", "varZero", "rowNoOcc", "transUnderflow", "nonqualGauss", "unusedStates"}
        elif cid == "e":
            assert have >= {"belowMinMix", "zeroWeight", "belowFloor", "ratioAboveOne", "noVarOcc", "noMuOcc", "varZero", "rowNoOcc", "transUnderflow", "unusedStates"}
        else:
            assert have == everything, (cid, everything - have)
        assert list(pl["nEgs"][:3]) == [0, 0, 1]
        pf = _stats(cid, "floors")[1]
        assert {"varBelow", "varOnFloor", "varUlpAbove"} <= set(pf)
    assert list(_stats("a", "minegs3")[1]["nEgs"][:3]) == [0, 2, 3] and list(_stats("a", "minegs0")[1]["nEgs"][:3]) == [0, 0, 0]


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if CONFIGS[c][1]])
@pytest.mark.parametrize("cid", CASE_IDS)
def test_restatement_equals_oracle(oracle, cid, cfg):
    """The numpy restatement against orc_update (pinned to the reference's HERest by test_oracle_golden.py): every array and the three
    counters the oracle returns, bit for bit."""
    pk = _set(cid)
    pc, qc, sc = _restated(cid, cfg)
    po, qo, so = uu.oracle_update(oracle, pk, uu.layout(pk), _stats(cid, cfg)[0], **_kw(cfg, int(pk["vecSize"])))
    for k in po:
        assert uu.same_bits(po[k], pc[k]), (k, int((np.asarray(po[k]).reshape(-1) != pc[k].reshape(-1)).sum()))
    for k in qo:
        assert uu.same_bits(qo[k], qc[k]), k
    assert so == {k: sc[k] for k in so}
    _planted_edges(pk, _stats(cid, cfg)[1], _kw(cfg, int(pk["vecSize"])), pc, qc, sc)


# ------------------------------------------------------------------------------------------------ the planted edges, by index
def _planted_edges(pk, pl, kw, p, q, st):
    """What each planted statistic must have done to the parameters `p`, the prepared tables `q` and the counters `st`."""
    p0 = uu.start_params(pk)
    off = pk["stateCompOff"]
    flags, single = kw.get("uFlags", UPALL), kw.get("singleProcess", False)
    mixes = bool(flags & UPMIXES) and int(np.diff(off).max()) > 1
    same = lambda k, idx: uu.same_bits(p[k][idx], p0[k][idx])
    untouched = lambda g: same("mean", g) and (single or (same("var", g) and same("gconst", g)))
    for s in pl["unusedStates"]:                               # anyS = 0: nothing moves, not even through singleProcess' round trips
        sl = slice(off[s], off[s + 1])
        assert same("mean", sl) and same("var", sl) and same("gconst", sl) and same("compWeight", sl), s
        assert all(q["compLogWt"][c] == uu.mix_log_weight(p0["compWeight"][c]) for c in range(off[s], off[s + 1]))
    for g in pl["nonqualGauss"]:                               # reached through models below minEgs (or without examples) only
        assert untouched(g), g
    for g in pl["atMinEgsGauss"]:                              # nEgs == minEgs qualifies, but not with 0 examples
        assert same("mean", g) == (not (kw["minEgs"] > 0 and flags & UPMEANS)), g
    for t in pl["deadTrans"]:
        assert same("transP", slice(pk["transOff"][t], pk["transOff"][t + 1])), t
    assert st["nSkippedHmm"] == pl["expect"]["nSkippedHmm"]
    assert st["nWeightAboveOne"] == 0
    if mixes:
        assert st["nNoMixUse"] == pl["expect"]["nNoMixUse"]
        for key in ("belowMinMix", "zeroWeight"):
            if key in pl and kw.get("mixWeightFloor", 0) == 0:     # (FloorMixes lifts it to the floor: a live component again)
                c = pl[key]
                assert p["compWeight"][c] == 0 and q["compLogWt"][c] == F(LZERO) and untouched(c), (key, c)
        if "ratioAboveOne" in pl:
            assert p["compWeight"][pl["ratioAboveOne"]] == (1 if kw.get("mixWeightFloor", 0) == 0 else p["compWeight"][pl["ratioAboveOne"]])
            if kw.get("mixWeightFloor", 0) == 0:
                assert q["compLogWt"][pl["ratioAboveOne"]] == 0
        if "stateNoOcc" in pl:
            s = pl["stateNoOcc"]
            assert single or same("compWeight", slice(off[s], off[s + 1]))
        if kw.get("mixWeightFloor", 0) > 0:
            fl = F(kw["mixWeightFloor"])
            for c in pl.get("belowFloor", []) + [pl[k] for k in ("belowMinMix", "zeroWeight") if k in pl]:
                assert p["compWeight"][c] == fl, c
            if "stateAllBelow" in pl:
                s = pl["stateAllBelow"]
                assert (p["compWeight"][off[s]:off[s + 1]] == fl).all()
            if "stateNoneBelow" in pl:                         # fsum == 0: the ratios as they are
                s = pl["stateNoneBelow"]
                assert (p["compWeight"][off[s]:off[s + 1]] > fl).all()
    else:
        assert st["nNoMixUse"] == 0
        if not single:
            assert same("compWeight", slice(None))
    if flags & UPTRANS:
        assert st["nNoTransOut"] == pl["expect"]["nNoTransOut"]
        assert p["transP"][pl["transUnderflow"]] == F(LZERO) and p0["transP"][pl["transUnderflow"]] > -0.5e10
        t, i = pl["rowNoOcc"]
        row = slice(pk["transOff"][t] + (i - 1) * 7, pk["transOff"][t] + i * 7)
        assert same("transP", row)
    else:
        assert st["nNoTransOut"] == 0 and same("transP", slice(None))
    g1, g2, g3 = pl["noVarOcc"], pl["noMuOcc"], pl["varGauss"]
    assert st["nNoVarUse"] == (1 if flags & UPVARS else 0)
    assert single or same("var", g1)
    assert same("mean", g1) == (not flags & UPMEANS)
    assert same("mean", g2) and (not flags & UPVARS or not same("var", g2))
    if flags & UPVARS:
        if "varZero" in pl:
            elems = pl["varZero"] if flags & UPMEANS else pl["varZero"][2:]      # (without the mean-shift term only the last one is 0)
            for g, k in elems:
                assert p["var"][g, k] == 0 and q["ivar"][g, k] == F(1) / F(1e-30), (g, k)
            assert p["gconst"][g3] < -0.5e10                   # a term of LZERO
            if flags & UPMEANS:
                assert st["nFloorVar"] == len(pl["varFloored"]) and st["nFloorVarMix"] == 1
            else:
                assert st["nFloorVar"] == 0 and st["nFloorVarMix"] == 0
        else:
            fl = _floors(kw, int(pk["vecSize"]))
            assert p["var"][pl["varBelow"]] == fl[0] and p["var"][pl["varOnFloor"]] == fl[1]
            assert p["var"][pl["varUlpAbove"]] == np.nextafter(fl[2], F(np.inf))
            assert st["nFloorVar"] >= 1 and st["nFloorVarMix"] >= 1
    else:
        assert st["nFloorVar"] == 0 and (single or same("var", slice(None)))


# ------------------------------------------------------------------------------------------------ on the device
def _log_rule(x, y, what):
    """Arrays behind a double log / exp on the device: the rule of test_device_update_equals_host_update.  -> entries that differ"""
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    ne = x != y
    print("%s: %d of %d entries differ" % (what, int(ne.sum()), x.size))
    assert ne.sum() <= max(3, 1e-5 * x.size), (what, int(ne.sum()))
    assert np.allclose(x[ne], y[ne], rtol=2.5e-7, atol=0), what
    assert np.array_equal(x < -0.5e10, y < -0.5e10), what     # LZERO (or a sum with a term of it) on one side is one on the other
    return int(ne.sum())


def _device_matches_host(mh, md, sh, sd, single, what):
    assert sh == sd, (sh, sd)
    ph, pd, qh, qd = mh.get_params(), md.get_params(), mh.get_prepared(), md.get_prepared()
    exact = [("mean", ph, pd), ("var", ph, pd), ("ivar", qh, qd)] + ([] if single else [("compWeight", ph, pd)])
    for k, x, y in exact:
        assert uu.same_bits(x[k], y[k]), (what, k, int((x[k].reshape(-1) != y[k].reshape(-1)).sum()))
    assert np.array_equal(qh["minDur"], qd["minDur"])
    n = {k: _log_rule(ph[k], pd[k], "%s %s" % (what, k)) for k in ("transP", "gconst") + (("compWeight",) if single else ())}
    n["compLogWt"] = _log_rule(qh["compLogWt"], qd["compLogWt"], "%s compLogWt" % what)
    assert uu.same_bits(pd["gconst"], qd["gconst"])
    return pd, qd, n


def _score(model, X, states, mode):
    from htk_amd import capi
    try:
        return model.outp_block(X, states, mode=mode)
    except capi.HtkAmdError as e:                              # fp16 tables: a variance of 0 is outside their range, for both models
        assert mode == 32 and e.rc == capi.ERANGE, e
        return np.zeros(0, F)


def _tables_match_fresh_model(native, oracle, pk, md, pd):
    """The scoring tables the update refreshed against those of a model created from the updated parameters."""
    D, S = int(pk["vecSize"]), int(pk["numStates"])
    pk2 = dict(pk, **{k: pd[k] for k in ("mean", "var", "gconst", "compWeight", "transP")})
    fresh = native.Model(pk2)
    X = np.random.default_rng(9).normal(0, 2.0, (70, D)).astype(F)          # one full 64-frame pass and a ragged one
    states = np.arange(S, dtype=np.int32)
    for mode in [0] + ([1] if D <= 40 else []) + ([4, 32] if D <= 48 else []):
        got, ref = _score(md, X, states, mode), _score(fresh, X, states, mode)
        assert got.shape == ref.shape and uu.same_bits(got, ref), mode
        if mode == 0:
            assert uu.same_bits(got, oracle.Model(pk2).score_block(X, states))


def _run_pair(native, pk, vec, kw):
    mh, md = native.Model(pk), native.Model(pk)
    acch, accd = native.Accs(mh), native.Accs(md)
    lay = uu.layout(pk)
    assert all(getattr(accd.lay, k) == lay[k] for k in lay)
    sh = mh.update(acch, vec, **kw)
    accd.upload_add(vec)
    sd = md.update_device(accd, **kw)
    return mh, md, sh, sd, accd


@gpu
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("cid", CASE_IDS)
def test_update_kernels(native, oracle, cid, cfg):
    """Each case under each configuration: host C update == restatement (== oracle where it applies) bit for bit; the device against the
    host: mean, var, ivar, minDur, counters and compWeight equal, the arrays behind a double log / exp by the project's rule; every
    planted edge by index; the refreshed scoring tables against a model created from the result.

    id  D   Ms (per state)          G    exercises
    a   13  1..4 cycled             67   state_w<4>, fused<1>, G mod 64 = 3, G D mod 4 = 3, lay.va even
    b   16  1..4 cycled             67   fused<1>, statistics by scalar loads (G odd, D even)
    c   26  5, 16, 1, 9 cycled      131  state_w<16>, fused<2>, 3 workgroups with a last one of 3
    d   39  17, 64, 2, 33, 3, ...   163  state_w<64>, fused<3>, last word cut short
    e   64  65, 1, 3                69   k_upd_trans + k_upd_state, fused<4> at its LDS maximum
    f   49  3, 2, 4 cycled          63   fused<4>, a single partial workgroup
    g   65  2..6 cycled             131  k_upd_gauss_elem + k_upd_gconst with LDS rows, G D mod 4 = 3
    h   97  1..3 cycled             129  k_upd_gconst taking the logs itself, second block of 1
    i   3   1..4 cycled             66   a 16-byte word spanning Gaussians in the fused kernel
    j   7   all 1                   70   no weight update; single-component closing constant of k_upd_mfma
    k   13  1..4 cycled             67   (a) with 257 transition matrices: two transition blocks behind one state block of 28 states
    (test_case_table_matches_the_launcher checks the rows against update.hip's thresholds.)"""
    pk = _set(cid)
    D = int(pk["vecSize"])
    kw = _kw(cfg, D)
    vec, pl = _stats(cid, cfg)
    mh, md, sh, sd, _ = _run_pair(native, pk, vec, kw)
    # the references among themselves
    ph, qh = mh.get_params(), mh.get_prepared()
    pc, qc, sc = _restated(cid, cfg)
    for k in pc:
        assert uu.same_bits(ph[k], pc[k]), ("host / restatement", k, int((ph[k].reshape(-1) != pc[k].reshape(-1)).sum()))
    for k in qc:
        assert uu.same_bits(qh[k], qc[k]), ("host / restatement", k)
    assert sh == sc, (sh, sc)
    if CONFIGS[cfg][1]:
        po, qo, so = uu.oracle_update(oracle, pk, uu.layout(pk), vec, **kw)
        assert all(uu.same_bits(po[k], ph[k]) for k in po) and all(uu.same_bits(qo[k], qh[k]) for k in qo), "host / oracle"
        assert so == {k: sh[k] for k in so}
    # the device
    pd, qd, n = _device_matches_host(mh, md, sh, sd, kw.get("singleProcess", False), "%s/%s" % (cid, cfg))
    _planted_edges(pk, pl, kw, pd, qd, sd)
    _tables_match_fresh_model(native, oracle, pk, md, pd)


@gpu
def test_ratio_above_1001_is_refused_alike(native):
    """A mixture weight ratio above 1.001 (HError 2393 in the reference): host and device refuse with the same error and count."""
    from htk_amd import capi
    pk = _set("d")
    vec, pl = _stats("d", "plain", above=True)
    mh, md = native.Model(pk), native.Model(pk)
    acch, accd = native.Accs(mh), native.Accs(md)
    accd.upload_add(vec)
    counts = []
    for call in (lambda: mh.update(acch, vec, minEgs=1), lambda: md.update_device(accd, minEgs=1)):
        with pytest.raises(capi.HtkAmdError) as e:
            call()
        assert e.value.rc == -5                                # HTKAMD_EMODEL
        counts.append(int(re.search(r"(\d+) mixture weights above 1.001", str(e.value)).group(1)))
    assert counts == [pl["expect"]["nWeightAboveOne"]] * 2


@gpu
def test_map_is_refused_on_the_device(native):
    from htk_amd import capi
    pk = _set("a")
    md = native.Model(pk)
    with pytest.raises(capi.HtkAmdError) as e:
        md.update_device(native.Accs(md), minEgs=1, uFlags=UPALL | capi.UPMAP)
    assert e.value.rc == -5


@gpu
def test_second_update_on_one_model_forgets_the_first(native):
    """Two updates in a row on one model object, the first with a varFloor vector, the second with none and other statistics, against a
    model that saw only the second from the same starting parameters: no stale mark, counter, floor vector or scratch block."""
    pk = _set("d")
    D = int(pk["vecSize"])
    vec1, _ = _stats("d", "floors")
    vec2, _ = uu.make_stats(pk, uu.layout(pk), 17, minEgs=2)
    md = native.Model(pk); acc = native.Accs(md)
    acc.upload_add(vec1)
    md.update_device(acc, **_kw("floors", D))
    p1 = md.get_params()
    md.set_params(**{k: np.asarray(v, F).reshape(p1[k].shape) for k, v in uu.start_params(pk).items()})
    acc.zero(); acc.upload_add(vec2)
    s2 = md.update_device(acc, minEgs=2)
    m2 = native.Model(dict(pk, gconst=uu.start_params(pk)["gconst"])); acc2 = native.Accs(m2)
    acc2.upload_add(vec2)
    r2 = m2.update_device(acc2, minEgs=2)
    assert s2 == r2, (s2, r2)
    a, b = md.get_params(), m2.get_params()
    assert all(uu.same_bits(a[k], b[k]) for k in a), [k for k in a if not uu.same_bits(a[k], b[k])]
    qa, qb = md.get_prepared(), m2.get_prepared()
    assert all(np.array_equal(qa[k], qb[k]) for k in qa)
    assert not uu.same_bits(a["var"], p1["var"])


@gpu
def test_update_in_two_halves_equals_the_whole(native):
    pk = _set("d")
    vec, _ = _stats("d", "minvar")
    kw = _kw("minvar", int(pk["vecSize"]))
    res = []
    for halves in (False, True):
        md = native.Model(pk); acc = native.Accs(md)
        acc.upload_add(vec)
        if halves:
            md.update_device_begin(acc, **kw)
            st = md.update_device_end()
        else:
            st = md.update_device(acc, **kw)
        res.append((st, md.get_params(), md.get_prepared()))
    assert res[0][0] == res[1][0]
    for k in (1, 2):
        assert all(uu.same_bits(res[0][k][n], res[1][k][n]) if res[0][k][n].dtype == F else np.array_equal(res[0][k][n], res[1][k][n]) for n in res[0][k])


@gpu
@pytest.mark.parametrize("cfg", ["plain", "single", "floors"])
def test_tied_vector_kernel_at_the_edges(native, cfg):
    """k_upd_gauss_elem_tied on case (d): groups of 2-4 Gaussians tied in mean and (other groups) in variance, a permuted scan order,
    no variance occupancy on a group's leader / on a member only / on a whole group, and groups of a Gaussian that only the model below
    minEgs reaches with Gaussians of qualifying models, that model first in the scan -- against the host update."""
    pk = dict(_set("d"))
    G, D = int(pk["numGauss"]), int(pk["vecSize"])
    kw = _kw(cfg, D)
    kw["minEgs"] = 2
    rng = np.random.default_rng(23)
    off = pk["stateCompOff"]
    vec, pl = uu.make_stats(pk, uu.layout(pk), 29, minEgs=2, floors=_floors(kw, D), mixFloor=MIXFLOOR)
    vec = vec.copy(); v = uu.views(pk, uu.layout(pk), vec)
    mean, var = np.array(pk["mean"], F).reshape(G, D), np.array(pk["var"], F).reshape(G, D)
    low = [g for s in uu.model_states(pk, 1) for g in range(off[s], off[s + 1])]              # model 1: minEgs - 1 examples
    assert set(low) <= set(pl["nonqualGauss"])
    ms, vs = np.full(G, -1, np.int32), np.full(G, -1, np.int32)
    groups = {}
    for share, vecs, name in ((ms, mean, "mu"), (vs, var, "va")):
        perm = [g for g in rng.permutation(G) if g not in low]
        pos, gid, groups[name] = 0, 0, []
        while pos < G // 2:
            n = int(rng.integers(2, 5))
            grp = np.array(sorted(perm[pos:pos + n])); pos += n
            if gid < len(low):
                grp = np.array(sorted([low[gid]] + list(grp)))[:4]
            share[grp] = gid; gid += 1
            vecs[grp] = vecs[grp.min()]
            groups[name].append(grp)
    pk["mean"], pk["var"] = mean, var
    good = {g for s in pl["qualStates"] if s != pl["stateNoOcc"] for g in range(off[s], off[s + 1])} - {pl["belowMinMix"], pl["zeroWeight"]} - set(low)
    ga, gb, gc = [grp for grp in groups["va"] if set(grp) <= good][-3:]                       # every member live in a qualifying state
    v["vaOcc"][ga[0]] = 0.0                                    # the leader alone
    v["vaOcc"][gb[-1]] = 0.0                                   # a member alone
    v["vaOcc"][gc] = 0.0                                       # the whole group: counted once
    order = np.concatenate([[1], rng.permutation([h for h in range(int(pk["numPhys"])) if h != 1])]).astype(np.int32)
    models = []
    for _ in range(2):
        m = native.Model(pk); m.set_sharing(ms, vs); m.set_scan_order(order)
        models.append(m)
    mh, md = models
    acch, accd = native.Accs(mh), native.Accs(md)
    sh = mh.update(acch, vec, **kw)
    accd.upload_add(vec)
    sd = md.update_device(accd, **kw)
    pd, qd, n = _device_matches_host(mh, md, sh, sd, kw.get("singleProcess", False), "tied/%s" % cfg)
    assert sd["nNoVarUse"] >= 1 and sd["nSkippedHmm"] == pl["expect"]["nSkippedHmm"]
    for name, k in (("mu", "mean"), ("va", "var")):
        for grp in groups[name]:
            assert (pd[k][grp] == pd[k][grp[0]]).all()
    p0 = dict(mean=mean, var=var)
    assert uu.same_bits(pd["var"][gc], var[gc]) or cfg == "single"
    assert not uu.same_bits(pd["var"][ga], var[ga]) and not uu.same_bits(pd["var"][gb], var[gb])
    assert not uu.same_bits(pd["mean"], p0["mean"])
