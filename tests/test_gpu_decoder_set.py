"""A batch decoded against a network per utterance (htkamd_decoder_set_*, DecoderSet; DoAlignment HVite.c:830): word alignment with
pronunciation variants as one launch, equality with the single decoder to the last bit, exact ties, failures beside successes, per-file
lattice rescoring against the reference's HVite, and the same through tools/bin/hvite."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from decode_util import GOLD, format_model_labels, format_words, load_decode_case, parse_opts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC, ALIGN, RESCORE = os.path.join(GOLD, "bigram"), os.path.join(GOLD, "align"), os.path.join(GOLD, "rescore")
FIELDS_I = ("wordPron", "wordStart", "wordEnd")
FIELDS_F = ("wordScore", "wordLm", "wordAc", "wordLike")


def _npz(path):
    z = np.load(path)
    return [z["u%d" % u] for u in range(len(z.files))]


def _bigram_set(native):
    mmf = native.Mmf(files=[os.path.join(SRC, "MMF")], hmm_list=os.path.join(SRC, "hmmlist"))
    return mmf, native.Model(mmf.packed())


def single_arrays(native, model, net, feats, order=None, maxWords=1024, **p):
    """htkamd_decoder_run_out of a decoder created for `net` alone: every output array, as DecoderSet.run_arrays returns them."""
    dec = native.Decoder(model, net, lmScale=p.get("lmScale", 1.0))
    if order is not None:
        dec.set_order(order)
    nU = len(feats)
    X = np.ascontiguousarray(np.concatenate(feats), np.float32)
    frameOff = np.concatenate([[0], np.cumsum([f.shape[0] for f in feats])]).astype(np.int32)
    dX = native.DevArray(X) if X.size else native.DevArray(nbytes=4)
    o = dict(nWords=np.zeros(nU, np.int32), wordPron=np.zeros((nU, maxWords), np.int32), wordStart=np.zeros((nU, maxWords), np.int32),
             wordEnd=np.zeros((nU, maxWords), np.int32), wordScore=np.zeros((nU, maxWords), np.float32), wordLm=np.zeros((nU, maxWords), np.float32),
             wordAc=np.zeros((nU, maxWords), np.float32), wordLike=np.zeros((nU, maxWords), np.float64), total=np.zeros(nU, np.float64),
             finalLm=np.zeros(nU, np.float32))
    out = native.DecodeOut(*[o[n].ctypes.data_as(C.c_void_p) for n, _ in native.DecodeOut._fields_])
    cfg = native.DecodeConfig(p.get("genBeam", 1.0e10), p.get("wordBeam", 1.0e10), p.get("lmScale", 1.0), p.get("wordPen", 0.0), p.get("prScale", 1.0), 0,
                              int(p.get("maxActive", 0)))
    native.check(native.lib().htkamd_decoder_run_out(dec.h, C.byref(cfg), dX.ptr, frameOff.ctypes.data_as(C.c_void_p), C.c_int(nU), C.c_int(maxWords), C.byref(out), None),
                 "decoder_run_out")
    return o, dec.last_tied()


def assert_same_as_single(native, model, nets, feats, net_of, order, what, maxWords=1024, **p):
    """One DecoderSet.run over (feats[u], nets[net_of[u]]) against a single decoder per network: == on the ints, array_equal on the floats
    and doubles.  Returns the set's arrays and its last_tied."""
    ds = native.DecoderSet(model, nets, lmScale=p.get("lmScale", 1.0))
    ds.set_order(order)
    got = ds.run_arrays(feats, net_of, maxWords=maxWords, **p)
    tied = 0
    for g in sorted(set(net_of)):
        us = [u for u in range(len(feats)) if net_of[u] == g]
        ref, t = single_arrays(native, model, nets[g], [feats[u] for u in us], order=order, maxWords=maxWords, **p)
        tied += t
        for k, u in enumerate(us):
            n = int(ref["nWords"][k])
            assert int(got["nWords"][u]) == n, (what, u, g)
            assert np.array_equal(got["total"][u], ref["total"][k]), (what, u, g)
            if n < 0:
                continue
            assert np.array_equal(got["finalLm"][u], ref["finalLm"][k]), (what, u, g)
            for f in FIELDS_I:
                assert [int(x) for x in got[f][u, :n]] == [int(x) for x in ref[f][k, :n]], (what, u, g, f)
            for f in FIELDS_F:
                assert got[f].dtype == ref[f].dtype and np.array_equal(got[f][u, :n], ref[f][k, :n]), (what, u, g, f)
    assert ds.last_tied() == tied, what
    return got, ds.last_tied()


def test_word_alignment_as_one_batch(native):
    """HVite -a from word-level transcriptions: every utterance of the `align` fixture in ONE DecoderSet.run, a network each; word-level and
    -m label lines are the reference's (formatted as tests/test_gpu_decode.py's per-utterance test formats them)."""
    from util import batch_arrays
    mmf, model = _bigram_set(native)
    feats = _npz(os.path.join(ALIGN, "feats.npz"))
    trans = json.load(open(os.path.join(ALIGN, "words.json")))
    expected = json.load(open(os.path.join(ALIGN, "expected.json")))
    n = variants = 0
    for opts, per in expected.items():
        p = parse_opts(opts)
        t = opts.split()
        bnd = t[t.index("-b") + 1] if "-b" in t else None
        nets = [native.Net(None, os.path.join(SRC, "dict"), mmf, words=w, boundary=bnd) for w in trans]
        ds = native.DecoderSet(model, nets, lmScale=p["lmScale"])
        res = ds.run(feats, list(range(len(feats))), **p)
        al = None
        if "-m" in t:
            chains = [np.array([m for w in words for m in nets[u].pron_models[w[0]]], np.int32) for u, (words, _) in enumerate(res)]
            Xb, frameOff, labOff, labs = batch_arrays([dict(seq=c, feat=f) for c, f in zip(chains, feats)])
            dX = native.DevArray(Xb)
            al = native.Viterbi(model).align(dX.ptr.value, frameOff, labOff, labs, genBeam=p["genBeam"])
        for u, (words, total) in enumerate(res):
            net = nets[u]
            assert [net.word_names[w[0]] for w in words] == ([bnd] if bnd else []) + trans[u] + ([bnd] if bnd else [])
            variants += sum(1 for w in words if net.pron_models[w[0]] == [0, 2])                 # AB's second pronunciation
            if al is not None:
                got = format_model_labels(words, ds.last_lm[u], al[u], net.pron_models, mmf.phys_names, net.word_names, p["lmScale"], p["wordPen"])
            else:
                got = format_words(words, net.out_syms)
            assert got == per["u%d" % u], (opts, u)
            n += len(got)
    assert n > 50 and variants > 0


def _model_sets(native):
    """The networks of the cases loop / tee / wint / ties and three alignment networks of different lengths, grouped by model set (MMF and
    model list): [(model, nets, [(features, network)])].  loop and the alignment networks share the `bigram` set."""
    groups = {}
    for case in ("loop", "tee", "wint", "ties"):
        d = os.path.join(GOLD, case)
        key = tuple(hashlib.md5(open(os.path.join(d, f), "rb").read()).hexdigest() for f in ("MMF", "hmmlist"))
        mmf, net, feats, _ = load_decode_case(native, case)
        g = groups.setdefault(key, dict(mmf=mmf, nets=[], utts=[]))
        g["nets"].append(net)
        g["utts"] += [(f, len(g["nets"]) - 1) for f in feats]
    key = tuple(hashlib.md5(open(os.path.join(SRC, f), "rb").read()).hexdigest() for f in ("MMF", "hmmlist"))
    g = groups[key]                                                # (the loop case's set)
    af = _npz(os.path.join(ALIGN, "feats.npz"))
    trans = json.load(open(os.path.join(ALIGN, "words.json")))
    for words, f in ((trans[1][:3], af[1][:45]), (trans[0], af[0]), (trans[3] + trans[2], np.concatenate([af[3], af[2]]))):
        g["nets"].append(native.Net(None, os.path.join(SRC, "dict"), g["mmf"], words=words))
        g["utts"].append((f, len(g["nets"]) - 1))
    g["utts"].append((af[0][:90], len(g["nets"]) - 2))             # a second utterance on the 6-word alignment network
    return [(native.Model(g["mmf"].packed()), g["nets"], g["utts"]) for g in groups.values()]


@pytest.fixture(scope="module")
def model_sets(native):
    return _model_sets(native)


@pytest.mark.parametrize("order", ["fast", "auto", "exact"])
def test_set_equals_single_decoder_bit_for_bit(native, model_sets, order):
    """Tee and plain models, networks from 8 nodes to the loop case's, netOf shuffled, networks shared by several utterances, with beams,
    scales and -u: every output of the set is the single decoder's."""
    mode = dict(fast=native.ORDER_FAST, auto=native.ORDER_AUTO, exact=native.ORDER_EXACT)[order]
    sizes = set()
    for gi, (model, nets, utts) in enumerate(model_sets):
        sizes |= set(n.desc.nNodes for n in nets)
        perm = np.random.default_rng(5 + gi).permutation(len(utts))
        feats, net_of = [utts[i][0] for i in perm], [utts[i][1] for i in perm]
        assert len(net_of) > len(set(net_of))                         # two utterances share a network
        for p in (dict(genBeam=250.0), dict(genBeam=60.0, wordBeam=30.0, lmScale=2.0, wordPen=3.0, prScale=2.0), dict(genBeam=250.0, maxActive=6)):
            assert_same_as_single(native, model, nets, feats, net_of, mode, (order, gi, sorted(p.items())), **p)
    assert min(sizes) < 20 <= max(sizes) and len(sizes) >= 6          # from a three-word alignment network to the loop case's


@pytest.mark.parametrize("order", ["auto", "exact"])
def test_set_chunk_boundaries_change_nothing(native, model_sets, order, monkeypatch):
    """The batches of the test above with one utterance per chunk, with uneven chunks of several and with one chunk (decode_util.CHUNK_BUDGETS):
    the outputs and last_tied of the run nobody cut.  In exact order a chunk of several utterances is grouped by network for the list kernel."""
    from decode_util import assert_same_decode_out, runs_under_chunk_budgets
    mode = dict(auto=native.ORDER_AUTO, exact=native.ORDER_EXACT)[order]
    for gi, (model, nets, utts) in enumerate(model_sets):
        perm = np.random.default_rng(5 + gi).permutation(len(utts))
        feats, net_of = [utts[i][0] for i in perm], [utts[i][1] for i in perm]
        ds = native.DecoderSet(model, nets)
        ds.set_order(mode)
        runs = runs_under_chunk_budgets(monkeypatch, lambda: (ds.run_arrays(feats, net_of, genBeam=250.0), ds.last_tied()))
        ref, tied = runs[0][1]
        assert tied == len(feats) or order == "auto"
        for budget, (got, t) in runs[1:]:
            assert_same_decode_out(got, ref, (order, gi, budget))
            assert t == tied, (order, gi, budget)


@pytest.mark.parametrize("case", ["ties2/tie_122", "ties2/tie_220"])
def test_set_exact_ties_go_through_the_list_kernel(native, case):
    mmf, net, feats, expected = load_decode_case(native, case)
    model = native.Model(mmf.packed())
    p = parse_opts(next(iter(expected)))
    per = expected[next(iter(expected))]
    net2 = load_decode_case(native, case)[1]                            # the same network a second time: two groups for the list kernel
    feats2, net_of = feats + feats[::-1], [0] * len(feats) + [1] * len(feats)
    got, tied = assert_same_as_single(native, model, [net, net2], feats2, net_of, native.ORDER_AUTO, case, **p)
    assert tied > 0
    ds = native.DecoderSet(model, [net, net2], lmScale=p["lmScale"])
    res = ds.run(feats2, net_of, **p)
    for u in range(len(feats)):
        assert format_words(res[u][0], net.out_syms) == per["u%d" % u], (case, u)
    got, tied = assert_same_as_single(native, model, [net, net2], feats2, net_of, native.ORDER_EXACT, case, **p)
    assert tied == len(feats2)


def test_failure_beside_success(native):
    mmf, model = _bigram_set(native)
    feats = _npz(os.path.join(ALIGN, "feats.npz"))
    trans = json.load(open(os.path.join(ALIGN, "words.json")))
    nets = [native.Net(None, os.path.join(SRC, "dict"), mmf, words=w) for w in trans]
    # beam 2: utterance 0 loses every token on its own network (at 5 it gets through), utterances 1 and 2 keep theirs
    order, net_of = [feats[1], feats[0], feats[2]], [1, 0, 2]
    got, _ = assert_same_as_single(native, model, nets, order, net_of, native.ORDER_AUTO, "beam", genBeam=2.0)
    assert [int(x) for x in got["nWords"]] == [6, -1, 6]
    wide, _ = assert_same_as_single(native, model, nets, order, net_of, native.ORDER_AUTO, "beam", genBeam=5.0)
    assert [int(x) for x in wide["nWords"]] == [6, 6, 6]
    # six words do not fit into maxWords = 4; the two-word networks on both sides do
    short = native.Net(None, os.path.join(SRC, "dict"), mmf, words=["E", "H"])
    got, _ = assert_same_as_single(native, model, [short, nets[0]], [feats[1][:30], feats[0], feats[2][:20]], [0, 1, 0], native.ORDER_AUTO, "maxWords", maxWords=4)
    assert [int(x) for x in got["nWords"]] == [2, -3, 2]
    # one frame: nothing reaches the end of a two-word network, and the neighbour is unaffected
    got, _ = assert_same_as_single(native, model, [short, nets[0]], [feats[1][:1], feats[0]], [0, 1], native.ORDER_AUTO, "T = 1")
    assert [int(x) for x in got["nWords"]] == [-1, 6]
    ds = native.DecoderSet(model, [short])
    assert ds.run([], []) == []
    with pytest.raises(native.HtkAmdError) as e:
        ds.run([feats[0]], [1])
    assert "names network 1 of 1" in str(e.value)
    with pytest.raises(native.HtkAmdError):
        ds.run([feats[0]], [-1])


def test_per_file_lattice_rescoring_against_hvite(native):
    """HVite -w (no name) -L dir -X lat: the reference wrote a lattice per utterance (-n 4 4 -z lat) and decoded each utterance against its
    own with other scales, penalties and beams (tests/golden/make_rescore_golden.py).  One set of six networks, one run per option set."""
    from util import batch_arrays
    mmf, model = _bigram_set(native)
    feats = _npz(os.path.join(RESCORE, "feats.npz"))
    expected = json.load(open(os.path.join(RESCORE, "expected.json")))
    nets = [native.Net(os.path.join(RESCORE, "lat", "u%d.lat" % u), os.path.join(SRC, "dict"), mmf) for u in range(len(feats))]
    assert len(nets) == 6 and len(expected) == 3
    for opts, per in expected.items():
        p = parse_opts(opts)
        ds = native.DecoderSet(model, nets, lmScale=p["lmScale"])
        res = ds.run(feats, list(range(len(feats))), **p)
        if "-m" in opts.split():
            chains = [np.array([m for w in words for m in nets[u].pron_models[w[0]]], np.int32) for u, (words, _) in enumerate(res)]
            Xb, frameOff, labOff, labs = batch_arrays([dict(seq=c, feat=f) for c, f in zip(chains, feats)])
            dX = native.DevArray(Xb)
            al = native.Viterbi(model).align(dX.ptr.value, frameOff, labOff, labs, genBeam=p["genBeam"])
        for u, (words, total) in enumerate(res):
            if "-m" in opts.split():
                got = format_model_labels(words, ds.last_lm[u], al[u], nets[u].pron_models, mmf.phys_names, nets[u].word_names, p["lmScale"], p["wordPen"])
            else:
                got = format_words(words, nets[u].out_syms)
            assert got == per["u%d" % u], (opts, u)


# ----------------------------------------------------------------------------------------- tools/bin/hvite
@pytest.fixture(scope="module")
def hvite(native):
    from htk_amd import build as nbuild
    nbuild.build_tools()
    exe = os.path.join(ROOT, "tools", "bin", "hvite")
    assert os.path.exists(exe)
    return exe


def _run(cmd, cwd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(cwd))


def _write_feats(d, feats):
    from htk_amd import synth
    for u, X in enumerate(feats):
        synth.write_htk_param(str(d / ("u%d.mfc" % u)), X, kind=9)
    (d / "scp").write_text("".join("u%d.mfc\n" % u for u in range(len(feats))))


def _mlf_text(per, n):
    return "#!MLF!#\n" + "".join('"u%d.rec"\n%s\n.\n' % (u, "\n".join(per["u%d" % u])) for u in range(n) if "u%d" % u in per)


def _align_files(tmp_path):
    feats = _npz(os.path.join(ALIGN, "feats.npz"))
    _write_feats(tmp_path, feats)
    for u, ws in enumerate(json.load(open(os.path.join(ALIGN, "words.json")))):
        (tmp_path / ("u%d.lab" % u)).write_text("\n".join(ws) + "\n")
    return len(feats), ["-H", os.path.join(SRC, "MMF")], [os.path.join(SRC, "dict"), os.path.join(SRC, "hmmlist")]


def test_hvite_cli_aligns_a_script_of_files_as_one_batch(hvite, tmp_path):
    n, pre, post = _align_files(tmp_path)
    expected = json.load(open(os.path.join(ALIGN, "expected.json")))
    assert any("-m" in o.split() for o in expected) and any("-m" not in o.split() for o in expected)
    for k, (opts, per) in enumerate(expected.items()):
        r = _run([hvite, "-a", "-S", "scp", "-i", "out%d.mlf" % k] + pre + opts.split() + post, tmp_path)
        assert r.returncode == 0, (opts, r.stderr)
        assert (tmp_path / ("out%d.mlf" % k)).read_text() == _mlf_text(per, n), opts
        # ... and in batches of three and one file: the same file
        r = _run([hvite, "-a", "--batch", "3", "-S", "scp", "-i", "b%d.mlf" % k] + pre + opts.split() + post, tmp_path)
        assert r.returncode == 0, (opts, r.stderr)
        assert (tmp_path / ("b%d.mlf" % k)).read_text() == _mlf_text(per, n), opts


def test_hvite_cli_rescoring_with_a_lattice_per_file(hvite, tmp_path):
    feats = _npz(os.path.join(RESCORE, "feats.npz"))
    _write_feats(tmp_path, feats)
    pre, post = ["-H", os.path.join(SRC, "MMF")], [os.path.join(SRC, "dict"), os.path.join(SRC, "hmmlist")]
    refs = sorted(f for f in os.listdir(RESCORE) if f.startswith("hvite__") and f.endswith(".mlf"))
    assert len(refs) == 3
    for fn in refs:
        opts = fn[len("hvite__"):-4].replace("_", " ").split()
        r = _run([hvite, "-S", "scp", "-i", "out.mlf", "-w", "-L", os.path.join(RESCORE, "lat"), "-X", "lat"] + pre + opts + post, tmp_path)
        assert r.returncode == 0, (fn, r.stderr)
        assert (tmp_path / "out.mlf").read_text() == open(os.path.join(RESCORE, fn)).read(), fn
    # -w "" is the same switch; two files that name one lattice share its network
    (tmp_path / "one").mkdir()
    r = _run([hvite, "-i", "same.mlf", "-w", "", "-L", os.path.join(RESCORE, "lat"), "-X", "lat"] + pre + refs[1][len("hvite__"):-4].replace("_", " ").split() + post
             + ["u1.mfc", "u1.mfc", "u0.mfc"], tmp_path)
    assert r.returncode == 0, r.stderr
    want = open(os.path.join(RESCORE, refs[1])).read().split('"u')
    assert (tmp_path / "same.mlf").read_text() == want[0] + '"u' + want[2] + '"u' + want[2] + '"u' + want[1]


@pytest.mark.parametrize("first", ["1.0", "2.0"])
def test_hvite_cli_alignment_retries_only_what_failed(hvite, tmp_path, first):
    """-a -t 1.0 50.0 151.0: at beam 1 files lose every token and are decoded again at 51 (DoAlignment HVite.c:900-913); the batch's MLF is
    what the files give one by one, and every file reports its own retries in file order.  At beam 1 all four files of the fixture need
    the wider beam; at beam 2 the oracle (oracle.decode, the reference's semantics on the CPU) loses file 0 alone, so that run has files
    that finish beside one that is decoded again."""
    n, pre, post = _align_files(tmp_path)
    beam = ["-t", first, "50.0", "151.0", "-m", "-T", "1"]
    r = _run([hvite, "-a", "-S", "scp", "-i", "all.mlf"] + pre + beam + post, tmp_path)
    assert r.returncode == 0, r.stderr
    alone, out = "#!MLF!#\n", ""
    for u in range(n):
        r1 = _run([hvite, "-a", "-i", "one%d.mlf" % u] + pre + beam + post + ["u%d.mfc" % u], tmp_path)
        assert r1.returncode == 0, r1.stderr
        alone += (tmp_path / ("one%d.mlf" % u)).read_text()[len("#!MLF!#\n"):]
        out += r1.stdout
    assert (tmp_path / "all.mlf").read_text() == alone
    assert r.stdout == out and "No tokens survived to final node of network at beam %s" % first in out
    assert out.count("at beam %s" % first) == (n if first == "1.0" else 1)
    assert out.count("File: ") == n                                   # every file got through at a wider beam
