"""htkamd_compv_full_cov (host/compv_full.c: CalcCovs in double, the inverse by Choleski) against float64 numpy.  No GPU."""
import numpy as np
import pytest


def stats(D, seed=3, n=200):
    X = np.random.default_rng(seed).standard_normal((n, D)) * np.linspace(1.0, 3.0, D) + 10.0
    return X, float(n), X.sum(0), (X.T @ X)[np.tril_indices(D)]


@pytest.mark.parametrize("D", [1, 13, 39])
def test_against_numpy(native, D):
    X, n, s, q = stats(D)
    mean, cov, inv = native.compv_full_cov(n, s, q)
    il = np.tril_indices(D)      # row-major (x, y), y <= x: the order of an MMF's <InvCovar>
    ref = np.cov(X.T, bias=True).reshape(D, D)
    # the arithmetic is double throughout (its error, times the condition number, is below 1e-12 here); what remains is the one
    # rounding of every result to float32, 2^-24 of itself
    assert np.allclose(mean, X.mean(0), rtol=1e-7, atol=0)
    assert np.allclose(cov, ref[il], rtol=1e-7, atol=1e-12)
    assert np.allclose(inv, np.linalg.inv(ref)[il], rtol=1e-7, atol=1e-12)


def test_floor_on_the_diagonal_only(native):
    D = 13
    X, n, s, q = stats(D)
    ref = np.cov(X.T, bias=True)
    floor = float(ref.diagonal().max()) * 2.0
    _, cov, _ = native.compv_full_cov(n, s, q, minVar=floor)
    full = np.zeros((D, D))
    full[np.tril_indices(D)] = cov
    assert (full.diagonal() == np.float32(floor)).all()
    off = np.tril_indices(D, -1)
    assert np.allclose(full[off], ref[off], rtol=1e-7, atol=1e-12)


def test_refusals(native):
    X, n, s, q = stats(13)
    with pytest.raises(native.HtkAmdError) as e:
        native.compv_full_cov(1.0, X[0], np.outer(X[0], X[0])[np.tril_indices(13)])
    assert e.value.rc == -1 and "2021" in str(e.value)
    X[:, 5] = X[:, 2]      # two equal columns: singular
    with pytest.raises(native.HtkAmdError) as e:
        native.compv_full_cov(n, X.sum(0), (X.T @ X)[np.tril_indices(13)])
    assert e.value.rc == -5 and "not positive definite" in str(e.value)
