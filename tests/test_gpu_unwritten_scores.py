"""No pass may read a score that the scoring kernels left unwritten.

The scoring kernels do not fill the score block: prep_utterance (csrc/fb.hip) cuts every task of chain states to the frames in which
Setotprob's ranges of the un-pruned pass can hold one of its models, and the bf16 pair kernels (csrc/gmm_bf16.hip, score modes 4 and 6)
leave out the (32 frames x pair of states) blocks outside both states' ranges.  The block lies in a buffer that grows and never shrinks,
so such a cell holds what the batch before left there.  Here the batch before is a poison batch P that writes EVERY cell the batch under
test B will occupy (every utterance of P is one non-tee model: with Q = 1 every task spans all frames and every state's range is the
whole utterance), once with scores as high as the set allows (P_hot: every frame the mean of a component of its state) and once with
scores thousands of nats lower (P_cold: those means plus 8 standard deviations in every dimension).  Both are ordinary finite scores of
an ordinary batch.  A read of an unwritten cell that reaches a result gives different results behind P_hot and behind P_cold; a read
that is discarded gives the same, and no baseline has to be trusted.
"""
import numpy as np
import pytest

from util import batch_arrays
from test_gpu_parity import PATHS, _chain_from_models

pytestmark = pytest.mark.gpu

MODES = [0, 4, 6]
# Started from the two settings of test_long_chains_every_kernel_class, (150, 0, 150) and (30, 60, 400).  The fixed beam of 150 stays: on
# this batch the oracle completes every utterance under it and its beta beam is narrower than the un-pruned one in most frames of the long
# chain.  (30, 60, 400) never retries here (B's frames lie close to their states' means: the oracle completes every utterance at a first
# beam of 2), so the retry setting starts at 1: alone that beam fails EVERY transcribed utterance of B, and the second attempt at 61
# completes them all -- StepBack's loop (HFB.c:1332-1361) runs a second beta pass over the same score block in every case.  All of this is
# asserted in build_world on the CPU and again on the device.
PRUNES = {"noprune": None, "beam": dict(pruneInit=150.0, pruneInc=0.0, pruneLim=150.0), "retry": dict(pruneInit=1.0, pruneInc=60.0, pruneLim=400.0)}
FIRST_BEAM_ALONE = dict(pruneInit=1.0, pruneInc=0.0, pruneLim=1.0)          # the retry setting without its increment

P_FRAMES = 400          # frames of every poison utterance
LONG, SKIP, TEE, SHORT, EMPTY, TAIL = range(6)          # B's utterances


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _poison_utt(pk, h, T, sigmas, k):
    """One model `h` over T frames: every frame the mean of a component of the state it visits, moved by `sigmas` standard deviations."""
    states = pk["hmmState"][pk["hmmStateOff"][h]:pk["hmmStateOff"][h + 1]]
    n = len(states)
    fr = []
    for j, s in enumerate(states):
        c0, c1 = int(pk["stateCompOff"][s]), int(pk["stateCompOff"][s + 1])
        c = c0 + (k + j) % (c1 - c0)
        x = pk["mean"][c].astype(np.float64) + sigmas * np.sqrt(pk["var"][c].astype(np.float64))
        fr += [x] * (T // n if j < n - 1 else T - (T // n) * (n - 1))
    return dict(seq=np.array([h], np.int32), feat=np.array(fr, np.float32))


def _cells(pk, utts):
    """sum of T x nSlots: what the batch takes of the score block"""
    emit = np.diff(pk["hmmStateOff"])
    return int(sum(len(u["feat"]) * int(emit[u["seq"]].sum()) for u in utts))


def _min_frames(pk, seq):
    """frames the chain needs at least: a model without a skip takes one per emitting state (the set's skip and tee models are not used here)"""
    return np.diff(pk["hmmStateOff"])[seq].sum()


def build_world(oracle):
    """Everything that needs no device: the set, batch B, the two poison batches, the oracle's passes over B under every pruning setting."""
    from htk_amd import synth
    pk, names, _, _ = synth.make_topo_set(seed=77, D=13, NU=1)
    a, b, sp, c, d, e = (names.index(n) for n in ("a", "b", "sp", "c", "d", "e"))
    emit = np.diff(pk["hmmStateOff"])
    rng = np.random.default_rng(20261)
    lr_models = [a, b, e, a, e, b, d, a, b, e, e, a, d, b, a, e, b, b, a, e, d, a, b, e, a, b, e, a, d, b]
    B = [None] * 6
    B[LONG] = _chain_from_models(rng, pk, lr_models)
    B[SKIP] = _chain_from_models(rng, pk, [b, c, a, e, c, b, d, a, c, e, b, a, c, e, b, a, e, b])
    B[TEE] = _chain_from_models(rng, pk, [a, sp, c, b, sp, e, a, b, sp, e, c, a, sp, b, e, a, sp, d, b, e])
    B[SHORT] = _chain_from_models(rng, pk, [d, a, d])
    B[EMPTY] = dict(seq=np.zeros(0, np.int32), feat=_chain_from_models(rng, pk, [b, e])["feat"])      # frames without a transcription
    B[TAIL] = _chain_from_models(rng, pk, [e, c, a, d, b])
    # the shapes the kernels' edges need
    assert len(lr_models) == 30 and not any(h in (sp, c) for h in lr_models)
    assert int(emit[B[LONG]["seq"]].sum()) > 64 and 128 < len(B[LONG]["feat"])          # two wide tasks of states (eleven exact ones), two tiles of frames
    assert c in B[SKIP]["seq"] and sp not in B[SKIP]["seq"]
    q = list(B[TEE]["seq"])
    assert sp in q and q[0] != sp and q[-1] != sp and not any(x == sp and y == sp for x, y in zip(q, q[1:]))
    assert len(B[SHORT]["seq"]) == 3 and len(B[SHORT]["feat"]) < 32
    assert sum(len(u["feat"]) for u in B[:EMPTY]) % 32 != 0 and len(B[EMPTY]["feat"]) > 0 and len(B[EMPTY]["seq"]) == 0
    assert all(len(B[u]["feat"]) >= 64 and len(B[u]["seq"]) >= 2 for u in (LONG, SKIP, TEE))
    # the poison: single non-tee models, enough of them to cover B's cells
    need = _cells(pk, B)
    P = {}
    for tag, sig in (("hot", 0.0), ("cold", 8.0)):
        P[tag] = []
        while _cells(pk, P[tag]) < need + 3 * P_FRAMES:
            k = len(P[tag])
            P[tag].append(_poison_utt(pk, (a, b, e)[k % 3], P_FRAMES, sig, k))
        assert all(len(u["seq"]) == 1 and u["seq"][0] != sp for u in P[tag])
        assert _cells(pk, P[tag]) >= need                                            # B sits entirely on P's cells
        assert np.isfinite(np.concatenate([u["feat"] for u in P[tag]])).all()
    # the oracle: B under every pruning setting (and the poison utterances are ordinary ones: they complete too)
    om = oracle.Model(pk)
    ora = {}
    for pid, prune in PRUNES.items():
        cfg = oracle.fb_cfg(**(prune or {}))
        res = []
        for ut in B:
            if len(ut["seq"]) == 0:
                res.append(None); continue
            rc, opr, dump = oracle.fb_utt(om, cfg, ut["feat"], ut["seq"], oracle.Accs(om), dump=True)
            assert rc == 1, (pid, rc)                                                 # every utterance with a transcription completes
            res.append(dict(pr=opr, qLo=dump["qLo"].copy(), qHi=dump["qHi"].copy()))
        ora[pid] = res
        for tag in P:
            for ut in P[tag][:3]:
                assert oracle.fb_utt(om, cfg, ut["feat"], ut["seq"], oracle.Accs(om))[0] == 1, (pid, tag)
    cfg = oracle.fb_cfg(**FIRST_BEAM_ALONE)
    for ut in B:                                                                      # the retry setting retries: its first beam alone fails every utterance
        assert not len(ut["seq"]) or oracle.fb_utt(om, cfg, ut["feat"], ut["seq"], oracle.Accs(om))[0] == 0
    assert FIRST_BEAM_ALONE["pruneInit"] == PRUNES["retry"]["pruneInit"] and PRUNES["retry"]["pruneInc"] > 0
    width = lambda r: r["qHi"] - r["qLo"]
    assert (width(ora["beam"][LONG]) < width(ora["noprune"][LONG])).any()            # the fixed beam does prune the long chain
    # the oracle's scores of every chain state (mode 0 is bit-exact against them)
    scores = []
    for ut in B:
        st = np.concatenate([pk["hmmState"][pk["hmmStateOff"][h]:pk["hmmStateOff"][h + 1]] for h in ut["seq"]] or [np.zeros(0, np.int32)])
        scores.append(om.score_block(ut["feat"], st.astype(np.int32)) if len(st) else None)
    # B with a transcription on the empty utterance's frames: a batch of B's size, whose per-frame words a context keeps when B follows
    B2 = list(B)
    B2[EMPTY] = dict(seq=np.array([d, a, d], np.int32), feat=B[EMPTY]["feat"])
    assert [len(u["feat"]) for u in B2] == [len(u["feat"]) for u in B] and int(_min_frames(pk, B2[EMPTY]["seq"])) <= len(B2[EMPTY]["feat"])
    return dict(pk=pk, B=B, B2=B2, P=P, ora=ora, scores=scores, emit=emit)


@pytest.fixture(scope="module")
def world(oracle):
    return build_world(oracle)


def _run(native, model, w, mode, path, prune, before, before_completes=True):
    """B on a context of its own, behind the batch `before` (or on the fresh context): what the pass leaves."""
    fb = native.ForwardBackward(model, debug=True, force_general=(path == "general"), no_state_path=(path == "wave"), no_lr_path=(path == "state"))
    cfg = native.fb_config(uFlags=15, scoreMode=mode, **(prune or {}))
    if before is not None:
        X, frameOff, labOff, labs = batch_arrays(before)
        dP = native.DevArray(X)
        fb.prepare(dP.ptr.value, frameOff, labOff, labs)
        fb.execute(cfg, native.Accs(model))
        st = fb.results()[1]
        assert not before_completes or (st == 1).all(), "the batch before is an ordinary batch: every utterance completes"
    X, frameOff, labOff, labs = batch_arrays(w["B"])
    dX = native.DevArray(X)
    acc = native.Accs(model)
    fb.prepare(dX.ptr.value, frameOff, labOff, labs)
    fb.execute(cfg, acc)
    pr, st = fb.results()
    tr = [fb.trellis(u) if len(ut["seq"]) else None for u, ut in enumerate(w["B"])]
    return dict(pr=np.array(pr), st=np.array(st), tr=tr, vec=acc.download()["vec"].copy())


def _same(got, ref, lay, H, what):
    """Results of two runs of B: pr, status, beams and every alpha / beta the trellis holds bit for bit, accumulators to the order of the atomics."""
    assert np.array_equal(_bits(got["pr"]), _bits(ref["pr"])) and np.array_equal(got["st"], ref["st"]), (what, got["pr"], ref["pr"], got["st"], ref["st"])
    for u, (g, r) in enumerate(zip(got["tr"], ref["tr"])):
        if r is None:
            assert g is None
            continue
        for k in ("qLo", "qHi", "aLo", "aHi"):
            assert np.array_equal(g[k], r[k]), (what, u, k)
        for k in ("beta", "alpha"):
            ng, nr = np.isnan(g[k]), np.isnan(r[k])
            assert np.array_equal(ng, nr), (what, u, k, "NaN pattern")
            bad = _bits(g[k])[~ng] != _bits(r[k])[~nr]
            assert not bad.any(), (what, u, k, int(bad.sum()), np.argwhere(~ng)[bad][:4].tolist())
    err = np.abs(got["vec"] - ref["vec"]) - (1e-12 * np.abs(ref["vec"]) + 1e-14)
    assert (err <= 0).all(), (what, int(np.argmax(err)), float(np.max(err)))
    for k in ("nEgs", "totalT", "nUttDone", "nUttSkipped", "nEval"):
        o = getattr(lay, k)
        n = H if k == "nEgs" else 1
        assert np.array_equal(got["vec"][o:o + n], ref["vec"][o:o + n]), (what, k)


@pytest.mark.parametrize("prune", list(PRUNES), ids=list(PRUNES))
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode", MODES, ids=["exact", "bf16x3", "bf16x3fast"])
def test_no_pass_reads_an_unwritten_score(native, oracle, world, monkeypatch, mode, path, prune):
    """Batch B behind P_hot, behind P_cold and on a fresh context (modes 4 and 6: also behind P_hot with HTKAMD_NO_TAPER_SKIP, the per-state
    skip off) gives one answer: `pr`, status, the four beams and every alpha / beta of the trellis bit for bit, accumulators within the
    summation-order noise of fp64 atomics (test_context_reused_batch_after_batch's bound), counters exactly; `pr` is the oracle's under the
    same pruning (1e-10 relative in mode 0 as test_forward_backward_vs_reference, 1e-6 in modes 4 and 6 as
    test_scoring_sits_out_what_setotprob_never_evaluates).  B: a left-to-right chain of 30 models (more than 64 chain states, more than 128
    frames), a chain with the skip model, one with the tee model inside, three models in fewer than 32 frames, frames without a
    transcription (skipped, its neighbours unchanged), and a short chain behind it.  Pruning: none, a fixed beam that narrows the long
    chain's beta beam, and a first beam that fails every utterance with an increment that completes it (PRUNES).

    The test sees what it looks for: cells whose hot and cold values differ are the ones the scorer did not write, they exist in every
    utterance of two models and 64 frames or more, and the per-state skip adds to them.  None of them lies where the reference evaluates
    (model q at frame t for qLo[t] - 1 <= q <= qHi[t], HFB.c:1014 with 1177 / 1215): those cells are bit-equal in all runs and, in mode 0,
    the oracle's score block.

    Measured share of unwritten cells (MI355X, every path and pruning setting alike): mode 0 29.7 % (8564 of 28876 cells); modes 4 and 6
    18.1 % (5218) with the per-state skip, 6.7 % (1948) without it."""
    w = world
    pk, B = w["pk"], w["B"]
    pr_cfg = PRUNES[prune]
    model = native.Model(pk)
    lay = native.accs_layout(pk)
    monkeypatch.delenv("HTKAMD_NO_TAPER_SKIP", raising=False)
    runs = {k: _run(native, model, w, mode, path, pr_cfg, p) for k, p in (("hot", w["P"]["hot"]), ("cold", w["P"]["cold"]), ("fresh", None))}
    if mode in (4, 6):
        monkeypatch.setenv("HTKAMD_NO_TAPER_SKIP", "1")
        runs["noskip"] = _run(native, model, w, mode, path, pr_cfg, w["P"]["hot"])
        monkeypatch.delenv("HTKAMD_NO_TAPER_SKIP", raising=False)
    fresh, hot, cold = runs["fresh"], runs["hot"], runs["cold"]

    # ---- the fresh run: every utterance with a transcription completes, the one without is skipped, pruning prunes, pr is the oracle's
    want = np.array([1 if len(ut["seq"]) else native.UTT_SKIPPED for ut in B], np.int32)
    assert np.array_equal(fresh["st"], want), fresh["st"]
    tol = 1e-10 if mode == 0 else 1e-6
    for u, o in enumerate(w["ora"][prune]):
        if o is not None:
            assert abs(fresh["pr"][u] - o["pr"]) <= tol * abs(o["pr"]), (u, fresh["pr"][u], o["pr"])
            if mode == 0:
                assert np.array_equal(fresh["tr"][u]["qLo"], o["qLo"]) and np.array_equal(fresh["tr"][u]["qHi"], o["qHi"]), u
    if prune == "beam":
        g, o = fresh["tr"][LONG], w["ora"]["noprune"][LONG]
        assert ((g["qHi"] - g["qLo"]) < (o["qHi"] - o["qLo"])).any()
    a = native.Accs(model).split(fresh["vec"])
    assert a["nUttDone"] == len(B) - 1 and a["totalT"] == sum(len(ut["feat"]) for ut in B if len(ut["seq"]))

    # ---- one answer
    for k, r in runs.items():
        if k != "fresh":
            _same(r, fresh, lay, int(pk["numPhys"]), "%s against fresh" % k)
    _same(hot, cold, lay, int(pk["numPhys"]), "hot against cold")

    # ---- what the scorer did not write, and where the reference evaluates
    nUnw = nUnwOff = nAll = 0
    for u, ut in enumerate(B):
        if not len(ut["seq"]):
            continue
        T, Q = len(ut["feat"]), len(ut["seq"])
        oh, oc, of = (_bits(runs[k]["tr"][u]["outp"]) for k in ("hot", "cold", "fresh"))
        emitting = ~np.isnan(hot["tr"][u]["outp"])                                     # [T, Q, maxN]: the chain's emitting states
        assert np.array_equal(emitting, ~np.isnan(cold["tr"][u]["outp"])) and emitting.sum() == T * int(w["emit"][ut["seq"]].sum())
        unw = (oh != oc) & emitting
        nAll += int(emitting.sum()); nUnw += int(unw.sum())
        if Q >= 2 and T >= 64:
            assert unw.any(), (u, "the poison is not in place: every cell of the utterance was written")
        if "noskip" in runs:
            on = _bits(runs["noskip"]["tr"][u]["outp"])
            assert np.array_equal(on[emitting & ~unw], oh[emitting & ~unw]), (u, "a score depends on the skip")
            nUnwOff += int((unw & (on == oh)).sum())                                   # (still the hot poison with the skip off)
        qLo, qHi = hot["tr"][u]["qLo"], hot["tr"][u]["qHi"]
        qs = np.arange(1, Q + 1)[None, :]
        ev = ((qs >= qLo[:, None] - 1) & (qs <= qHi[:, None]))[:, :, None] & emitting   # where Setotprob evaluates in this pass
        assert ev.any()
        assert not (unw & ev).any(), (u, int((unw & ev).sum()), np.argwhere(unw & ev)[:4].tolist())
        assert np.array_equal(oh[ev], of[ev]), u
        if mode == 0:
            ref = np.full(emitting.shape, np.nan, np.float32)
            ref[emitting] = w["scores"][u].reshape(-1)                                 # [t][q][state] in chain order, as `emitting` enumerates
            assert np.array_equal(oh[ev], _bits(ref)[ev]), u
    print("unwritten cells, mode %d %s %s: %d of %d (%.4f)%s" % (mode, path, prune, nUnw, nAll, nUnw / nAll,
          "; skip off: %d (%.4f)" % (nUnwOff, nUnwOff / nAll) if "noskip" in runs else ""))
    if "noskip" in runs:
        assert nUnw > nUnwOff, (nUnw, nUnwOff)


@pytest.mark.parametrize("path", PATHS)
def test_frames_without_transcription_behind_a_batch_of_the_same_size(native, world, path):
    """prepare refills the per-frame words (taperLo, taperHi, qBeamNP) only when the batch's frame count changes, so behind the poison
    batches B never sees stale ones.  Here the batch before is B itself with a transcription on the empty utterance's frames: same
    frame count, so the context keeps that utterance's words when B follows, and prep_utterance has to clear them for the frames that
    now have no transcription.  B gives what it gives on a fresh context, in the sense of the test above, under the retry setting --
    and on the device too that setting's first beam alone fails every transcribed utterance, so the passes compared here did retry."""
    w = world
    pk, B = w["pk"], w["B"]
    model = native.Model(pk)
    fresh = _run(native, model, w, 0, path, PRUNES["retry"], None)
    again = _run(native, model, w, 0, path, PRUNES["retry"], w["B2"], before_completes=False)      # (the words are laid at prepare, whatever the pass makes of the utterance)
    want = np.array([1 if len(ut["seq"]) else native.UTT_SKIPPED for ut in B], np.int32)
    assert np.array_equal(fresh["st"], want) and np.array_equal(again["st"], want)
    _same(again, fresh, native.accs_layout(pk), int(pk["numPhys"]), "B behind B with the empty utterance transcribed")
    alone = _run(native, model, w, 0, path, FIRST_BEAM_ALONE, None)
    assert (alone["st"] == native.UTT_SKIPPED).all(), alone["st"]
