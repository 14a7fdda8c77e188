"""htkamd_compv_full (csrc/compv_full.hip) against float64 numpy: S_k = sum_f w_f [x_f, 1]^T [x_f, 1] per class, at the tile edges of
D and the chunk edges of the frame count, over label segments, run to run, its refusals, and HCompV's FULLC flat start end to end.

The bound is the fp64 summation bound, not a measurement: |got - ref| <= 2 F 2^-53 sum_f |w_f x_fi x_fj| (the factor 2: the one
rounding of w x_i).  Inputs are multiples of 2^-10 below 64 in size, so without weights every product and sum is exact in fp64 and
count, sum and squares must equal numpy's bit for bit.

End to end (test_hcompv_fullc_example): the largest relative difference between a float32 restatement of AccVar / CalcCovs in file
order and the float64 one, on the golden data after the inversion, measured on the CPU by tests/golden/make_compv_full_golden.py, is
E2E_MEASURED = 3.487e-4; four times that is allowed (the inversion amplifies by the condition number and the restatement is not the
reference's compiler): 1.395e-3."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "compv_full")
U = 2.0 ** -53
E2E_MEASURED = 3.487e-4      # make_compv_full_golden.py --measure: the whole files' inverse covariance (the labelled case: 8.030e-05)
E2E_ALLOWED = 4 * E2E_MEASURED
DIMS = (1, 15, 16, 17, 39, 128)
FRAMES = {"1": lambda C: 1, "3": lambda C: 3, "4": lambda C: 4, "5": lambda C: 5, "C-1": lambda C: C - 1, "C": lambda C: C, "C+1": lambda C: C + 1,
          "2C+7": lambda C: 2 * C + 7}
CASES = [(D, "2C+7") for D in DIMS] + [(39, f) for f in FRAMES if f != "2C+7"]


def table(F, D, seed):
    """Cepstrum-like rows (|x| < 64, column offset 10) in multiples of 2^-10, and a weight per frame in (0, 2)."""
    rng = np.random.default_rng(seed)
    X = np.clip(np.round((rng.standard_normal((F, D)) * 8.0 + 10.0) * 1024.0) / 1024.0, -63.0, 63.0).astype(np.float32)
    return X, rng.uniform(0.01, 2.0, F).astype(np.float32)


def reference(X, w, rows):
    """count, sum, the full square matrix and the bound's sum of magnitudes over `rows`, in float64 with the weight on the row operand."""
    Xd = X[rows].astype(np.float64)
    wd = np.ones(len(Xd)) if w is None else w[rows].astype(np.float64)
    wx = wd[:, None] * Xd
    return wd.sum(), wx.sum(0), np.einsum("fi,fj->ij", wx, Xd), np.einsum("fi,fj->ij", np.abs(wx), np.abs(Xd)), np.abs(wx).sum(0), len(Xd)


def check_class(got, ref, D, exact):
    count, sum_, sq = got
    rn, rs, rq, mag, smag, F = ref
    il = np.tril_indices(D)
    if exact:
        assert count == rn and np.array_equal(sum_, rs) and np.array_equal(sq, rq[il])
    assert abs(count - rn) <= 2 * F * U * rn
    assert (np.abs(sum_ - rs) <= 2 * F * U * smag).all()
    err, lim = np.abs(sq - rq[il]), 2 * F * U * mag[il]
    assert (err <= lim).all(), (float(err.max()), float(lim[err.argmax()]), int(err.argmax()))


@pytest.mark.parametrize("weighted", [False, True], ids=["w1", "w"])
@pytest.mark.parametrize("D,frames", CASES)
def test_against_float64(native, D, frames, weighted):
    F = FRAMES[frames](native.compv_full_chunk())
    X, w = table(F, D, 100 * D + F)
    dX, dW = native.DevArray(X), native.DevArray(w)
    count, sum_, sq = native.compv_full(dX.ptr, F, D, weights_ptr=dW.ptr if weighted else None)
    check_class((count[0], sum_[0], sq[0]), reference(X, w if weighted else None, slice(None)), D, exact=not weighted)


@pytest.fixture(scope="module")
def segment_case(native):
    C, D, K = native.compv_full_chunk(), 39, 6
    F = 3 * C + 5
    X, w = table(F, D, 7)
    segs = [(0, 1, 0),                                   # one frame
            (10, 3, 1),                                  # shorter than one K step
            (5, C + 9, 2),                               # longer than a chunk: straddles a chunk boundary
            (100, 40, 3), (2 * C, 77, 3),                # two disjoint segments of one class
            (C + 10, 200, 1), (C + 100, 200, 4),         # overlapping segments of different classes
            (50, 0, 4)]                                  # empty; class 5 has no segment
    dX, dW = native.DevArray(X), native.DevArray(w)
    run = lambda: native.compv_full(dX.ptr, F, D, segs=segs, nClass=K, weights_ptr=dW.ptr)
    return X, w, segs, K, D, run


def test_segments(segment_case):
    X, w, segs, K, D, run = segment_case
    count, sum_, sq = run()
    for k in range(K):
        rows = np.concatenate([np.arange(a, a + n) for a, n, c in segs if c == k] + [np.zeros(0, np.int64)]).astype(np.int64)
        check_class((count[k], sum_[k], sq[k]), reference(X, w, rows), D, exact=False)
    assert count[5] == 0.0 and not sum_[5].any() and not sq[5].any()


def test_same_bytes_run_to_run(segment_case):
    run = segment_case[-1]
    a, b = run(), run()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("D,segs,nClass,reason", [(129, None, 1, "limit of 128"), (39, [(0, 8, 0), (60, 5, 0)], 1, "segment 1"), (39, [(0, 8, 2)], 2, "class 2")],
                         ids=["D129", "segment-past-end", "class-out-of-range"])
def test_refusals(native, D, segs, nClass, reason):
    F = 64
    dX = native.DevArray(np.zeros((F, D), np.float32))
    out = (np.full(nClass, 7.0), np.full((nClass, D), 7.0), np.full((nClass, D * (D + 1) // 2), 7.0))
    with pytest.raises(native.HtkAmdError) as e:
        native.compv_full(dX.ptr, F, D, segs=segs, nClass=nClass, out=out)
    assert e.value.rc == -1 and reason in str(e.value)
    assert all((a == 7.0).all() for a in out)


@pytest.mark.parametrize("labelled", [False, True], ids=["whole-files", "label-segments"])
def test_hcompv_fullc_example(native, tmp_path, labelled):
    """examples/hcompv_fullc.py on the golden files reproduces the mean and inverse covariance of the FULLC set the reference's HCompV
    wrote, within E2E_ALLOWED (see the module's docstring) relative to the largest entry of each."""
    scp = tmp_path / "train.scp"
    scp.write_text("".join(os.path.join(GOLD, n) + "\n" for n in sorted(os.listdir(GOLD)) if n.endswith(".mfc")))
    args = ["-l", "S", "-L", GOLD] if labelled else []
    spec = importlib.util.spec_from_file_location("hcompv_fullc", os.path.join(ROOT, "examples", "hcompv_fullc.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    example.main(["-m", "-M", str(tmp_path), "-S", str(scp)] + args + [os.path.join(GOLD, "proto")])
    got = native.Mmf(files=[str(tmp_path / "proto")]).packed()
    ref = native.Mmf(files=[os.path.join(GOLD, "hcompv_lab" if labelled else "hcompv_all", "proto")]).packed()
    for key in ("mean", "invCov"):
        g, r = np.asarray(got[key], np.float64), np.asarray(ref[key], np.float64)
        print(key, float(np.abs(g - r).max() / np.abs(r).max()))
        assert np.abs(g - r).max() <= E2E_ALLOWED * np.abs(r).max()
