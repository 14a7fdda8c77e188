"""N-best token sets and lattices with a network per utterance (htkamd_decoder_set_run_lattice[_align], DecoderSet.run_lattice; the SET
forms of k_decode_ord_n / k_decode_n): equality with the single decoder to the last bit over networks of very different sizes in one
launch, the oracle's lattices and the reference's files for the fixtures of tests/golden/decode/set_nbest, the static order, failures
beside successes, chunks, and the same through tools/bin/hvite."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from decode_util import runs_under_chunk_budgets
from set_nbest_util import ALIGN, INDEX, SETNB, SRC, TAGS, bigram_mmf, check_files, load_case, npz
from test_nbest_lattice import _arc_key

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mixed(native):
    """The loop network and three alignment networks of 3, 6 and 11 words over the `bigram` model set (tests/test_gpu_decoder_set.py's
    _model_sets), and a batch over them whose net_of is not monotone: two utterances share the loop network, the largest network (11
    words) stands next to the smallest (3 words).  (model, nets, feats, net_of)"""
    from test_gpu_decoder_set import _model_sets
    model, nets, utts = max(_model_sets(native), key=lambda g: len(g[1]))
    loop, a3, a6, a11 = 0, len(nets) - 3, len(nets) - 2, len(nets) - 1
    sizes = [nets[g].desc.nNodes for g in (loop, a3, a6, a11)]
    assert sizes[1] == min(sizes) and sizes[3] == max(sizes) and sizes[3] > 4 * sizes[1], sizes
    of = lambda g: [f for f, n in utts if n == g]
    mine = [nets[g] for g in (loop, a3, a6, a11)]
    feats = [of(a6)[0], of(loop)[0], of(a11)[0], of(a3)[0], of(loop)[1]]
    return model, mine, feats, [2, 0, 3, 1, 0]


def _same(got, ref, what):
    assert (got is None) == (ref is None), what
    if ref is None:
        return
    assert sorted(got) == sorted(ref), what
    for k in ref:
        assert np.asarray(got[k]).dtype == np.asarray(ref[k]).dtype and np.array_equal(got[k], ref[k]), (what, k)


@pytest.mark.parametrize("nToks,order,align", [(2, "ORDER_AUTO", 0), (8, "ORDER_AUTO", 0), (2, "ORDER_EXACT", 0), (8, "ORDER_EXACT", 0), (3, "ORDER_AUTO", 3)])
def test_set_lattices_equal_the_single_decoders_bit_for_bit(native, mixed, nToks, order, align):
    model, nets, feats, net_of = mixed
    order = getattr(native, order)
    ds = native.DecoderSet(model, nets)
    ds.set_order(order)
    got = ds.run_lattice(feats, net_of, nToks, genBeam=250.0, align=align)
    assert ds.last_tied() == len(feats)
    arcs = 0
    for g in sorted(set(net_of)):
        us = [u for u in range(len(feats)) if net_of[u] == g]
        dec = native.Decoder(model, nets[g])
        dec.set_order(order)
        ref = dec.run_lattice([feats[u] for u in us], nToks, genBeam=250.0, align=align)
        for k, u in enumerate(us):
            assert ref[k] is not None
            _same(got[u], ref[k], (nToks, order, u, g))
            arcs += len(ref[k]["arcStart"])
    assert arcs > 5 * len(feats)


def _arcs(l):
    return sorted(zip(l["arcStart"].tolist(), l["arcEnd"].tolist(), l["arcAc"].tolist(), l["arcLm"].tolist(), l["arcPr"].tolist(), l["arcScore"].tolist()))


def _recs(l, model_of):
    out = []
    for j in range(len(l["arcStart"])):
        a0, a1 = int(l["arcAlignOff"][j]), int(l["arcAlignOff"][j + 1])
        out.append((int(l["arcStart"][j]), int(l["arcEnd"][j]), float(l["arcScore"][j]),
                    tuple((int(l["alState"][q]), int(model_of(l, q)), int(l["alDur"][q]), float(l["alLike"][q])) for q in range(a0, a1))))
    return sorted(out)


@pytest.fixture(scope="module")
def refs(native, oracle):
    """tag -> (case, nets, feats, parameters, alignment mode, the oracle's lattice per utterance): computed once, read by several tests."""
    mmf = bigram_mmf(native)
    om = oracle.Model(mmf.packed())
    out = {"mmf": mmf, "model": native.Model(mmf.packed())}
    for tag in TAGS:
        c, nets, feats, p, align = load_case(native, mmf, tag)
        out[tag] = (c, nets, feats, p, align, [oracle.decode_nbest(om, X, net.arrays(), c["nToks"], align=align, **p) for X, net in zip(feats, nets)])
    return out


@pytest.mark.parametrize("tag", TAGS)
def test_set_kernel_equals_oracle_and_hvite(native, refs, tag, tmp_path):
    """Every fixture case as ONE DecoderSet.run_lattice: the oracle's lattice per utterance (total, nodes, sorted arcs, the -m records value
    for value), then the reference's files.  rescore_u is maxActive through the set, one utterance of it without a surviving token."""
    c, nets, feats, p, align, ref = refs[tag]
    ds = native.DecoderSet(refs["model"], nets, lmScale=p["lmScale"])
    lats = ds.run_lattice(feats, list(range(len(feats))), c["nToks"], align=align, **p)
    assert ds.last_tied() == len(feats)
    for u, (got, r) in enumerate(zip(lats, ref)):
        assert (got is None) == (r is None) == ("u%d" % u not in c["nbest"]), (tag, u)
        if r is None:
            continue
        assert got["total"] == r["total"], (tag, u)
        for k in ("nodeFrame", "nodeNet", "nodeLike"):
            assert np.array_equal(got[k], r[k]), (tag, u, k)
        assert _arcs(got) == _arcs(r), (tag, u)
        if align:
            am = nets[u].arrays()["model"]
            assert _recs(got, lambda l, q: l["alModel"][q]) == _recs(r, lambda l, q: am[l["alNode"][q]]), (tag, u)
    assert sum(l is None for l in lats) == (1 if tag == "rescore_u" else 0)
    for u, got in enumerate(lats):
        if got is not None:
            check_files(native, got, nets[u], refs["mmf"], tag, u, tmp_path)


@pytest.mark.parametrize("tag", [t for t in TAGS if not INDEX[t]["lab"]])
def test_set_kernel_static_order_matches_oracle(native, refs, tag):
    """k_decode_n<DEC_SET_THREADS, true>: the oracle's best token exactly, its arcs, their acoustic scores to 1e-3 -- the project's own
    tolerance for this kernel (test_token_set_kernel_static_order_matches_oracle: relative likelihoods re-based in another association)."""
    c, nets, feats, p, align, ref = refs[tag]
    ds = native.DecoderSet(refs["model"], nets, lmScale=p["lmScale"])
    ds.set_order(native.ORDER_FAST)
    lats = ds.run_lattice(feats, list(range(len(feats))), c["nToks"], **p)
    assert ds.last_tied() == 0
    for u, (got, r) in enumerate(zip(lats, ref)):
        assert (got is None) == (r is None), (tag, u)
        if r is None:
            continue
        assert got["total"] == r["total"], (tag, u)
        g, q = _arc_key(got), _arc_key(r)
        assert [x[:5] for x in g] == [x[:5] for x in q], (tag, u)
        assert np.allclose([x[5] for x in g], [x[5] for x in q], atol=1e-3), (tag, u)
    with pytest.raises(native.HtkAmdError, match="ORDER_FAST"):
        ds.run_lattice(feats, list(range(len(feats))), c["nToks"], align=1, **p)


def test_set_lattice_edge_cases(native, mixed):
    model, nets, feats, net_of = mixed
    ds = native.DecoderSet(model, nets)
    assert ds.run_lattice([], [], 3) == []
    res = ds.run_lattice([feats[0], feats[3][:1], feats[3]], [2, 1, 1], 3, genBeam=250.0)
    assert res[0] is not None and res[1] is None and res[2] is not None        # one frame cannot reach the end of a three-word network
    with pytest.raises(native.HtkAmdError, match="does not fit"):
        ds.run_lattice([feats[0]], [2], 3, genBeam=250.0, maxNodes=4)
    for bad in (-1, len(nets)):
        with pytest.raises(native.HtkAmdError, match="names network") as e:
            ds.run_lattice([feats[0], feats[3]], [2, bad], 3)
        assert e.value.rc == -1
    with pytest.raises(native.HtkAmdError, match="nToks = 9"):
        ds.run_lattice([feats[0]], [2], 9)


def test_set_lattices_do_not_depend_on_the_chunks_of_the_batch(native, mixed, monkeypatch):
    model, nets, feats, net_of = mixed
    ds = native.DecoderSet(model, nets)
    runs = runs_under_chunk_budgets(monkeypatch, lambda: (ds.run_lattice(feats, net_of, 3, genBeam=250.0), ds.last_tied()))
    ref, tied = runs[0][1]
    assert tied == len(feats) and all(l is not None and len(l["arcStart"]) > 0 for l in ref)
    for budget, (got, t) in runs[1:]:
        assert t == tied, budget
        for u, (g, r) in enumerate(zip(got, ref)):
            _same(g, r, (budget, u))


@pytest.mark.parametrize("tag", TAGS)
def test_hvite_writes_the_references_files(native, tag, tmp_path):
    """tools/bin/hvite with the switches the reference's HVite was given (tests/golden/make_set_nbest_golden.py), in a directory laid out
    as the reference's was: the master label file and every lattice byte for byte, no lattice for an utterance without a surviving token."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_set_nbest_golden as gen
    from htk_amd import build as nbuild
    nbuild.build_tools()
    c = INDEX[tag]
    gen.lay_out(str(tmp_path))
    r = subprocess.run([os.path.join(ROOT, "tools", "bin", "hvite"), "-C", "config", "-H", "MMF"] + gen.switches(c) + ["dict", "hmmlist"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "out.mlf").read() == open(os.path.join(SETNB, tag, "out.mlf")).read(), tag
    for u in range(c["n"] if c["latExt"] else 0):
        name = "u%d.%s" % (u, c["latExt"])
        if "u%d" % u not in c["nbest"]:
            assert not os.path.exists(tmp_path / "out" / name) and "No tokens survived" in r.stderr, (tag, u)
            continue
        assert open(tmp_path / "out" / name).read() == open(os.path.join(SETNB, tag, name)).read(), (tag, u)
