"""The binding's batch helper (capi.offsets, capi._pack: the host half of capi._Batch) without a device, and on the device the one path
that came to use it with another C entry point: Decoder.run through htkamd_decoder_run_out."""
import numpy as np
import pytest

from decode_util import load_decode_case


def test_offsets_are_the_int32_exclusive_prefix_sum(native):
    for lengths, want in (([], [0]), ([0], [0, 0]), ([1, 3], [0, 1, 4]), ((2, 0, 5), [0, 2, 2, 7]), (np.array([4, 4], np.int64), [0, 4, 8])):
        got = native.offsets(lengths)
        assert got.dtype == np.int32 and got.tolist() == want, lengths


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_pack_of_no_array_and_of_an_array_without_rows(native, dtype):
    host, off = native._pack([], dtype, cols=3)
    assert host.shape == (0, 3) and host.dtype == dtype and off.tolist() == [0]
    host, off = native._pack([], dtype)                                   # no column count: an empty vector
    assert host.shape == (0,) and host.dtype == dtype and off.tolist() == [0]
    for cols in (3, None):
        host, off = native._pack([np.zeros((0, 3))], dtype, cols=cols)
        assert host.shape == (0, 3) and host.dtype == dtype and off.tolist() == [0, 0]


def test_pack_puts_the_arrays_one_behind_the_other(native):
    a, b = np.arange(3, dtype=np.float32).reshape(1, 3), 10 + np.arange(9, dtype=np.float32).reshape(3, 3)
    host, off = native._pack([a, b], np.float32, cols=3)
    assert host.dtype == np.float32 and host.flags.c_contiguous and off.dtype == np.int32 and off.tolist() == [0, 1, 4]
    assert np.array_equal(host, np.concatenate([a, b]))
    waves, off = native._pack([np.array([5], np.int16), np.array([-1, 2, 3], np.int16)], np.int16)      # vectors give a vector
    assert waves.dtype == np.int16 and waves.tolist() == [5, -1, 2, 3] and off.tolist() == [0, 1, 4]


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_pack_makes_strided_float64_input_contiguous_and_typed(native, dtype):
    big = np.arange(48, dtype=np.float64).reshape(6, 8)
    strided, transposed = big[::2, ::2], np.asfortranarray(big[:1, :4])            # [3, 4] and [1, 4], neither C-contiguous float32
    assert not strided.flags.c_contiguous
    host, off = native._pack([transposed, strided], dtype, cols=4)
    assert host.dtype == dtype and host.flags.c_contiguous and host.shape == (4, 4) and off.tolist() == [0, 1, 4]
    assert np.array_equal(host, np.concatenate([transposed, strided]).astype(dtype))
    one, off = native._pack([strided], dtype)                                       # a single array is copied too, never a view
    assert one.dtype == dtype and one.flags.c_contiguous and one.base is not big and np.array_equal(one, strided.astype(dtype))
    column, off = native._pack([big[:, 0]], dtype)                                  # a strided vector
    assert column.dtype == dtype and column.flags.c_contiguous and column.tolist() == big[:, 0].tolist() and off.tolist() == [0, 6]


def test_pack_refuses_a_mismatched_column_count_in_its_caller_s_name(native):
    ok, bad = np.zeros((2, 3), np.float32), np.zeros((2, 4), np.float32)
    for arrays, cols in (([ok, bad], None), ([ok, bad], 3), ([ok], 4), ([np.zeros(3, np.float32)], 3), ([np.float32(1.0)], None)):
        with pytest.raises(native.HtkAmdError, match="^Decoder.run: array"):
            native._pack(arrays, np.float32, cols=cols, who="Decoder.run")
    with pytest.raises(native.HtkAmdError, match="^batch: array 1 "):
        native._pack([np.zeros(2, np.int16), np.zeros((2, 1), np.int16)], np.int16)


def test_the_qualifier_wrappers_refuse_an_empty_list_by_name(native):
    quals = native.parm_quals_from_kind("MFCC_E_D", 13)
    with pytest.raises(native.HtkAmdError, match="^parm_add_qualifiers: "):
        native.parm_add_qualifiers([])
    with pytest.raises(native.HtkAmdError, match="^parm_qualify: "):
        native.parm_qualify([], quals)
    with pytest.raises(native.HtkAmdError, match="^InputXForm.apply: "):
        native.InputXForm.apply(None, [], quals)


@pytest.mark.gpu
def test_decoder_run_equals_decoder_set_run_and_an_empty_batch_is_an_empty_result(native):
    """Decoder.run, now through htkamd_decoder_run_out and the shared unpacker, on two utterances of the `loop` network (80 frames each, six
    words each) against DecoderSet.run over that single network: pron, start, end, score, total and last_lm with ==, as the header promises
    the two entry points the same bits.  The same for the arrays of run_arrays.

    An empty `feats` list, as found on the commit before the shared holder (MI355X): none of the four raises.  Decoder.run([]) returned []
    and left last_lm = []; Decoder.run_lattice([], 2) returned []; DecoderSet.run([], []) returned [] and left last_lm = [] and
    last_status = []; DecoderSet.run_lattice([], [], 2) returned [].  The same is asserted here."""
    mmf, net, feats, _ = load_decode_case(native, "loop")
    model = native.Model(mmf.packed())
    dec, ds = native.Decoder(model, net), native.DecoderSet(model, [net])
    feats = feats[:2]
    got, ref = dec.run(feats), ds.run(feats, [0, 0])
    assert len(got) == len(ref) == 2 and ds.last_status == [len(w) for w, _ in ref]
    for u, ((gw, gt), (rw, rt)) in enumerate(zip(got, ref)):
        assert rw is not None and len(rw) > 1, u                        # a real path, so there is something to compare
        assert len(gw) == len(rw), u
        for g, r in zip(gw, rw):
            assert g[0] == r[0] and g[1] == r[1] and g[2] == r[2] and g[3] == r[3], (u, g, r)
        assert gt == rt, u
    assert dec.last_lm == ds.last_lm and [len(x) for x in dec.last_lm] == [len(w) for w, _ in ref]
    ga, ra = dec.run_arrays(feats), ds.run_arrays(feats, [0, 0])
    assert list(ga) == list(ra)
    for k in ra:
        n = ra["nWords"]
        assert ga[k].dtype == ra[k].dtype and ga[k].shape == ra[k].shape, k
        assert all(np.array_equal(ga[k][u, :n[u]], ra[k][u, :n[u]]) if ra[k].ndim == 2 else ga[k][u] == ra[k][u] for u in range(2)), k

    assert dec.run([]) == [] and dec.last_lm == []
    assert dec.run_lattice([], 2) == []
    assert ds.run([], []) == [] and ds.last_lm == [] and ds.last_status == []
    assert ds.run_lattice([], [], 2) == []
