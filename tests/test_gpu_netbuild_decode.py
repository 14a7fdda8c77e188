"""A network built in memory goes to the decoder without a file: labels counted on the device, the bigram model, HBuild's back-off network
and its expansion over tests/golden/decode/bigram's dictionary and models give the label files that the same decoder gives over the
reference-built SLF of that model (tests/golden/lm/decode7/bo.slf)."""
import os

import pytest

from htk_amd import capi
from decode_util import GOLD, format_words
import lm_cases as lc
import numpy as np

pytestmark = pytest.mark.gpu


def test_in_memory_network_decodes_like_the_reference_slf(native, tmp_path):
    src = os.path.join(GOLD, "bigram")
    d, words, utts, manifest = lc.load_case("decode7")
    dic = tmp_path / "dict"
    dic.write_text(open(os.path.join(src, "dict")).read() + "!ENTER [] p0\n!EXIT [] p1\n")
    mmf = native.Mmf(files=[os.path.join(src, "MMF")], hmm_list=os.path.join(src, "hmmlist"))
    z = np.load(os.path.join(src, "feats.npz"))
    feats = [z["u%d" % u] for u in range(len(z.files))]

    ls = capi.LabelStats(words)
    ids, _ = lc.case_ids(ls, utts)
    ls.count(ids).bigram_write(str(tmp_path / "bo"), backoff=True)
    assert (tmp_path / "bo").read_bytes() == open(os.path.join(d, "bo.bigram"), "rb").read()
    wordnet = capi.Network.from_bigram(capi.Bigram(str(tmp_path / "bo")), words + ["!ENTER", "!EXIT"])
    mem = wordnet.expand(str(dic), mmf)
    ref = native.Net(os.path.join(d, "bo.slf"), str(dic), mmf)
    a, b = mem.arrays(), ref.arrays()
    assert all(np.array_equal(a[k], b[k]) for k in a) and mem.out_syms == ref.out_syms

    model = native.Model(mmf.packed())
    for lm_scale in (1.0, 5.0):
        got = native.Decoder(model, mem, lmScale=lm_scale).run(feats, genBeam=250.0, wordBeam=1.0e10, lmScale=lm_scale, wordPen=0.0, prScale=1.0)
        want = native.Decoder(model, ref, lmScale=lm_scale).run(feats, genBeam=250.0, wordBeam=1.0e10, lmScale=lm_scale, wordPen=0.0, prScale=1.0)
        assert any(w is not None for w, _ in want)
        for (gw, gt), (ww, wt) in zip(got, want):
            assert (gw is None) == (ww is None) and gt == wt
            if ww is not None:
                assert format_words(gw, mem.out_syms) == format_words(ww, ref.out_syms)
