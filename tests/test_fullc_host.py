"""Full-covariance (FULLC) model files on the host: <INVCOVAR> read in text and binary form, gConst as the reference forms it, written
back byte-identically to the reference's re-saves, and every construct the path does not serve refused by name.  Fixtures:
tests/golden/make_fullc_golden.py."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FC = os.path.join(GOLD, "fullc")
LST = os.path.join(GOLD, "demo", "bcplist")
D = 26


def covdet_gconst(tri, D):
    """FixFullGConst(mp, -CovDet(inv)): Choleski in double, log-det summed in float (LogFloat), D*log(2 pi) + that, stored to float."""
    L = np.zeros((D, D))
    for i in range(D):
        for j in range(i + 1):
            s = float(tri[i * (i + 1) // 2 + j])
            for k in range(j):
                s -= L[i, k] * L[j, k]
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    ld = np.float32(0.0)
    for j in range(D):
        ld = np.float32(float(ld) + np.log(L[j, j]))
    return np.float32(D * np.log(6.28318530717959) + float(-np.float32(2.0 * float(ld))))


def test_text_and_binary_read_to_the_same_set(native):
    a = native.Mmf(files=[os.path.join(FC, "fullc_in")], hmm_list=LST).packed()
    b = native.Mmf(files=[os.path.join(FC, "fullc_in_bin")], hmm_list=LST).packed()
    assert a["covKind"] == "FULLC" and a["invCov"].shape == (15, D * (D + 1) // 2)
    assert a["var"] is None                                  # no variances in the description: htkamd_model_create refuses it
    assert np.array_equal(a["invCov"], b["invCov"]) and np.array_equal(a["mean"], b["mean"])
    # the text file carries HERest's gConsts, the binary re-save HHEd's recomputation from the stored inverse
    rec = np.array([covdet_gconst(t, D) for t in a["invCov"]], np.float32)
    assert np.array_equal(rec, b["gconst"])
    assert np.allclose(a["gconst"], rec, rtol=1e-5, atol=0)
    # the triangle is packed row-major: a symmetric matrix with the file's diagonal
    full = np.zeros((D, D), np.float32)
    full[np.tril_indices(D)] = a["invCov"][0]
    assert (np.diag(full) > 0).all() and np.count_nonzero(np.tril(full, -1)) > D


def test_missing_gconst_is_computed_as_the_reference_does(native):
    s = native.Mmf(files=[os.path.join(FC, "seed")], hmm_list=LST).packed()
    assert s["gconst"] is not None
    assert np.array_equal(s["gconst"], np.array([covdet_gconst(t, D) for t in s["invCov"]], np.float32))


def test_written_back_byte_identical(native, tmp_path):
    m = native.Mmf(files=[os.path.join(FC, "fullc_in")], hmm_list=LST)
    pk = m.packed()
    pk["gconst"] = np.array([covdet_gconst(t, D) for t in pk["invCov"]], np.float32)      # what HHEd's re-save holds
    m.write(pk, one_file=str(tmp_path / "t"))
    m.write(pk, one_file=str(tmp_path / "b"), binary=True)
    assert (tmp_path / "t").read_bytes() == open(os.path.join(FC, "fullc_resaved"), "rb").read()
    assert (tmp_path / "b").read_bytes() == open(os.path.join(FC, "fullc_in_bin"), "rb").read()
    # the source-preserving writer, binary
    m.write_sources(pk, [str(tmp_path / "s")], binary=True)
    assert (tmp_path / "s").read_bytes() == open(os.path.join(FC, "fullc_in_bin"), "rb").read()
    # parameters without the inverse covariances: an error that names them, not a KeyError
    for call in (lambda q: m.write(q, one_file=str(tmp_path / "u")), lambda q: m.write_sources(q, [str(tmp_path / "v")])):
        with pytest.raises(native.HtkAmdError, match="invCov"):
            call(dict(pk, invCov=None))


def test_diagonal_writer_refuses_a_fullc_set_and_back(native, tmp_path):
    m = native.Mmf(files=[os.path.join(FC, "fullc_in")], hmm_list=LST)
    pk = m.packed()
    L = native.lib()
    with pytest.raises(native.HtkAmdError, match="FULLC"):
        native.check(L.htkamd_mmf_write(m.h, native._p(pk["mean"]), native._p(pk["mean"]), native._p(pk["gconst"]), native._p(pk["compWeight"]),
                                        native._p(pk["transP"]), str(tmp_path / "x").encode(), None), "mmf_write")
    d = native.Mmf(files=[os.path.join(GOLD, "demo", "hmm_final", n) for n in open(LST).read().split()])
    dp = d.packed()
    assert "invCov" not in dp and d.cov_kind == "DIAGC"
    with pytest.raises(native.HtkAmdError, match="not FULLC"):
        native.check(L.htkamd_mmf_write_full(d.h, native._p(dp["mean"]), native._p(dp["var"]), native._p(dp["gconst"]), native._p(dp["compWeight"]),
                                             native._p(dp["transP"]), str(tmp_path / "y").encode(), None, 0), "mmf_write_full")


def test_model_create_refuses_the_description_of_a_fullc_set(native):
    """The flat description carries no covariance kind: a FULLC set's has no variances, so the DIAGC constructor cannot take it silently
    (checked ahead of the device: this holds on a machine without one)."""
    m = native.Mmf(files=[os.path.join(FC, "fullc_in")], hmm_list=LST)
    h = native.C.c_void_p()
    rc = native.lib().htkamd_model_create(native.C.byref(m.desc), native.C.byref(h))
    assert rc != 0 and not h
    assert b"htkamd_model_create_full" in native.lib().htkamd_last_error()


HDR = "~o <STREAMINFO> 1 2 <VECSIZE> 2 <NULLD><USER>%s\n"
TRANS = "<TRANSP> 3\n0 1 0\n0 .5 .5\n0 0 0\n<ENDHMM>\n"
INV = "<INVCOVAR> 2\n2 0.5\n1\n"
VAR = "<VARIANCE> 2\n1 1\n"


def hmm(name, body):
    return '~h "%s"\n<BEGINHMM>\n<NUMSTATES> 3\n<STATE> 2\n%s%s' % (name, body, TRANS)


def test_fullc_sets_that_are_refused(native, tmp_path):
    ok = HDR % "<FULLC>" + hmm("a", "<MEAN> 2\n0 0\n" + INV)
    p = tmp_path / "ok"; p.write_text(ok)
    pk = native.Mmf(files=[str(p)]).packed()
    assert np.array_equal(pk["invCov"][0], np.array([2, 0.5, 1], np.float32))         # file order (0,0) (1,0) | (1,1) -> packed (0,0) (1,0) (1,1)
    bad = {      # name: (text, what the message must name)
        "shared_inverse": (HDR % "<FULLC>" + '~i "c"\n' + INV, "~i (shared inverse covariance)"),
        "shared_inverse_use": (HDR % "<FULLC>" + hmm("a", '<MEAN> 2\n0 0\n~i "c"\n'), "~i (shared inverse covariance)"),
        "shared_mean": (HDR % "<FULLC>" + '~u "m"\n<MEAN> 2\n0 0\n' + hmm("a", '<NUMMIXES> 1\n<MIXTURE> 1 1.0\n~u "m"\n' + INV), "~u / ~v vector sharing inside a FULLC set"),
        "shared_var_macro": (HDR % "<FULLC>" + '~v "v"\n' + VAR + hmm("a", "<MEAN> 2\n0 0\n" + INV), "~u / ~v vector sharing inside a FULLC set"),
        "mixed": (HDR % "<FULLC>" + hmm("a", "<MEAN> 2\n0 0\n" + INV) + hmm("b", "<MEAN> 2\n0 0\n" + VAR), "mixes <VARIANCE> and <INVCOVAR>"),
        "fullc_over_variances": (HDR % "<FULLC>" + hmm("a", "<MEAN> 2\n0 0\n" + VAR), "mixes <VARIANCE> and <INVCOVAR>"),
        "streams": ("~o <STREAMINFO> 2 1 1 <VECSIZE> 2 <NULLD><USER><FULLC>\n" +
                    hmm("a", "<NUMMIXES> 1 1\n<STREAM> 1\n<MEAN> 1\n0\n<INVCOVAR> 1\n1\n<STREAM> 2\n<MEAN> 1\n0\n<INVCOVAR> 1\n1\n"), "FULLC together with <STREAMINFO>"),
        "not_pd": (HDR % "<FULLC>" + hmm("a", "<MEAN> 2\n0 0\n<INVCOVAR> 2\n1 2\n1\n"), "not positive definite"),
        "lltc": (HDR % "<LLTC>", "only DIAGC and FULLC covariances"),
        "xformc": (HDR % "<XFORMC>", "only DIAGC and FULLC covariances"),
        "invdiagc": (HDR % "<INVDIAGC>", "only DIAGC and FULLC covariances"),
        "lltcovar": (HDR % "<FULLC>" + hmm("a", "<MEAN> 2\n0 0\n<LLTCOVAR> 2\n1 0\n1\n"), "only DIAGC and FULLC covariances"),
    }
    for name, (text, what) in bad.items():
        p = tmp_path / name
        p.write_text(text)
        with pytest.raises(native.HtkAmdError) as e:
            native.Mmf(files=[str(p)])
        assert what in str(e.value), (name, str(e.value))
    # the variance floor macro stays allowed in a FULLC set
    p = tmp_path / "vfloor"; p.write_text(HDR % "<FULLC>" + '~v "varFloor1"\n<VARIANCE> 2\n0.1 0.1\n' + hmm("a", "<MEAN> 2\n0 0\n" + INV))
    m = native.Mmf(files=[str(p)])
    assert m.cov_kind == "FULLC" and np.allclose(m.var_floor, [0.1, 0.1])


def test_tied_mixture_fullc_is_refused(native, tmp_path):
    pool = '~m "TM_1_1"\n<MEAN> 2\n0 0\n%s~m "TM_1_2"\n<MEAN> 2\n1 1\n%s'
    body = '<NUMMIXES> 2\n<TMIX> "TM_1_"\n 0.5 0.5\n'
    p = tmp_path / "tmix_diag"; p.write_text(HDR % "<DIAGC>" + pool % (VAR, VAR) + hmm("a", body))
    assert native.Mmf(files=[str(p)]).packed()["hsKind"] == 1        # the same set with variances is a tied-mixture set
    p = tmp_path / "tmix"; p.write_text(HDR % "<FULLC>" + pool % (INV, INV) + hmm("a", body))
    with pytest.raises(native.HtkAmdError, match="FULLC together with <TMIX>"):
        native.Mmf(files=[str(p)])


def test_diagonal_set_reads_as_before(native):
    d = native.Mmf(files=[os.path.join(GOLD, "demo", "hmm_final", n) for n in open(LST).read().split()])
    pk = d.packed()
    assert d.inv_cov is None and "covKind" not in pk and pk["var"].shape == (15, D)
    assert (pk["var"] > 0).all() and not np.all(pk["var"] == 1.0)
