"""Split R-hat without a device: the Python twin (tests/rhat_model.py) of the facade's rhat_estimator against the facade itself
(tests/cxx/rhat_fixture_main.cc, bit for bit), against a vectorised textbook evaluation, and on cases whose answers are known."""
import tempfile

import numpy as np
import pytest

import rhat_model as R


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def ar1(n, ns, nf, seed, offset=0.0):
    """stationary AR(1) series [n, ns, nf] of unit variance"""
    rng = np.random.default_rng(seed)
    phi = rng.uniform(0.1, 0.9, size=(ns, nf))
    e = rng.standard_normal((n, ns, nf)) * np.sqrt(1 - phi * phi)
    x = np.empty_like(e)
    cur = rng.standard_normal((ns, nf))
    for t in range(n):
        cur = phi * cur + e[t]
        x[t] = cur
    return x + offset


@pytest.fixture(scope="module")
def fixture_exe():
    with tempfile.TemporaryDirectory() as d:
        yield R.build_fixture_driver(d)


@pytest.mark.parametrize("W", [1, 3, 70])
@pytest.mark.parametrize("nfeat", [1, 3])
def test_the_facade_estimator_and_the_twin_agree_bit_for_bit(fixture_exe, W, nfeat):
    series = ar1(90, W, nfeat, seed=100 * W + nfeat, offset=3.0)
    for nrows in (4, 34, 90):
        want = R.split_rhat(R.series_window(series, nrows), detail=True)
        got = R.fixture_driver_answers(fixture_exe, series, nrows)
        for name, g, w in zip(("rhat", "mean", "within", "between", "seq_mean", "seq_var"), got, want):
            assert same_bits(g, w), (W, nfeat, nrows, name, np.ravel(g)[:4], np.ravel(w)[:4])
        assert np.isfinite(got[0]).all() and (got[0] > 0.7).all()


@pytest.mark.parametrize("shape", [(400, 70, 3), (40, 1, 1), (250, 7, 2), (1000, 50, 2)])
def test_twin_agrees_with_the_textbook_evaluation(shape):
    """N <= 1e5 samples, means and variances of order 1: N * 2^-52 times the condition of the sums is about 2e-11"""
    series = ar1(*shape, seed=7, offset=2.0)
    assert series.size <= 1e5
    got, want = R.split_rhat(series), R.textbook(series)
    for name, g, w in zip(("rhat", "mean", "within", "between"), got, want):
        assert np.all(np.abs(g - w) <= 1e-10 * np.abs(w)), (shape, name, g, w)


def test_a_series_far_from_zero_keeps_the_answer_of_the_centred_data():
    """offset 1e6, unit variance: the two-pass variance loses nothing; a sum-of-squares form misses this by about 1e-4"""
    centred = ar1(500, 20, 2, seed=11)
    got = R.split_rhat(centred + 1.0e6)
    want = R.textbook(centred)
    print(got[0], want[0])
    assert np.all(np.abs(got[0] - want[0]) <= 1e-9 * want[0])
    assert np.all(np.abs(got[2] - want[2]) <= 1e-9 * want[2])
    # the sum-of-squares form on the same data is off by far more than the bound: the check can tell the two apart
    x = R.split(centred + 1.0e6)
    n = x.shape[0]
    naive_var = (np.sum(x * x, axis=0) - n * np.mean(x, axis=0) ** 2) / (n - 1)
    assert np.abs(np.mean(naive_var, axis=0) - want[2]).max() > 1e-7 * want[2].max()


def test_equal_sequences_have_no_between_variance():
    x = R.equal_sequences()
    n = x.shape[0] // 2
    rhat, mean, within, between = R.split_rhat(x)
    assert (between == 0).all() and (mean == 3).all() and within.tolist() == [2.0, 8.0]
    assert same_bits(rhat, np.full(2, np.sqrt((n - 1.0) / n)))


def test_two_groups_ten_sigma_apart_do_not_agree():
    rhat, _, within, between = R.split_rhat(R.two_groups())
    print(rhat)
    assert (rhat > 2).all() and (np.abs(rhat - 5.0) < 0.5).all()     # var_plus ~ within * (1 + 25)


def test_a_constant_feature_gives_the_ieee_result():
    x = ar1(20, 3, 2, seed=5)
    x[:, :, 1] = 2.5
    rhat = R.split_rhat(x)[0]
    assert np.isfinite(rhat[0]) and np.isnan(rhat[1])               # 0 / 0
