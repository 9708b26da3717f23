"""tests/ess_model.py -- the Python restatement of the facade's ess_estimator that checks the device's effective-sample-size
kernels -- against the real reference's answers (tests/golden/ess.json.gz) and, bit for bit, against the facade's own estimator
(tests/cxx/de_ess_fixture_main.cc); and the C ABI's new names."""
import os
import tempfile

import numpy as np
import pytest

import ess_model as M
import golden_io

ESS_NAMES = ["ptm_ess_windowed", "ptm_ess_report", "ptm_ess_series_windowed", "ptm_ess_series_report", "ptm_ess_last_on_device"]


@pytest.fixture(scope="module")
def golden():
    g = golden_io.load("ess.json.gz")
    out = []
    for c in g["cases"]:
        series = M.golden_series(c)
        est = M.Estimator(c["n"], 1, c["dim"], M.series_reader(series[:, None, :]))
        out.append((c, series, [est.report(q["width"], q["every"], q["esslimit"], c["n"], 0) for q in c["queries"]]))
    return out


def test_model_reproduces_the_reference_answers(golden):
    nonzero = 0
    for c, _, answers in golden:
        for q, (ess, length) in zip(c["queries"], answers):
            assert int(length[0]) == q["length"], (q, ess, length)
            assert abs(ess[0] - q["ess"]) <= 1e-10 * max(1.0, abs(q["ess"])), (q, ess)
            nonzero += q["ess"] > 0
    assert nonzero >= 15


def test_model_equals_the_facade_estimator_bit_for_bit(golden):
    with tempfile.TemporaryDirectory() as d:
        exe = M.build_fixture_driver(d)
        for c, series, answers in golden:
            host = M.fixture_driver_answers(exe, series, c["queries"])
            for q, (ess, length), (h_ess, h_len) in zip(c["queries"], answers, host):
                assert int(length[0]) == h_len, (q, length, h_len)
                assert np.float64(ess[0]).tobytes() == np.float64(h_ess).tobytes(), (q, float(ess[0]), h_ess)


def test_model_skips_samples_the_ring_has_lost():
    """the validity hook: a reader that misses some steps gives the sums of the samples that are there, in their order"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((400, 1, 2))
    gone = np.zeros(400, dtype=bool)
    gone[[130, 131, 250, 399]] = True

    def read(steps):
        return ~gone[steps][:, None], x[steps]
    est = M.Estimator(400, 1, 2, read)
    nwin, lags, mean, cov, count = est.table(50, 1, 2)
    assert nwin == 6 and lags[:3] == [0, 1, 2]
    w, l = 5, 2                                   # window of steps 350..399, lag 2
    s1 = s2 = np.zeros(2)
    n = 0
    for i in range(350, 400):
        if gone[i] or gone[i - 2]:
            continue
        s1 = s1 + (x[i - 2, 0] + x[i, 0])
        s2 = s2 + x[i - 2, 0] * x[i, 0]
        n += 1
    assert n == 49 and count[w, l, 0] == n
    mu = s1 / n / 2
    assert np.array_equal(mean[w, l, 0], mu) and np.array_equal(cov[w, l, 0], s2 / n - mu * mu)


def test_header_declares_the_ess_entry_points_and_the_binding_exports_them():
    from test_abi_cpu import declared_functions
    from ptmcmc_amd import engine as E
    names = declared_functions()
    for n in ESS_NAMES:
        assert n in names, n
        assert n in E.EXPORTS, n
    assert sorted(E.EXPORTS) == names
    for n in ("effective_samples", "ess_windowed"):
        assert callable(getattr(E.Engine, n))
    assert callable(E.effective_samples_series) and callable(E.ess_series_windowed)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_series_calls_fail_loudly_without_a_gpu():
    from ptmcmc_amd import engine as E
    with pytest.raises(E.PtmError) as ei:
        E.effective_samples_series(np.zeros((100, 1, 1)), 10, 1)
    assert "no gfx950" in str(ei.value)
