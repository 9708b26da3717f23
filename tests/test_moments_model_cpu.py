"""Pooled posterior moments without a device: the Python twin (tests/moments_model.py) of the facade's moments_estimator against the
facade itself (tests/cxx/moments_main.cc, bit for bit) and against np.cov; the C ABI's declarations, exports and early refusals; the
covariance file's round trip and refusals; and the estimator and the file code under the address and undefined-behaviour sanitizers
(a stand-alone host program)."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest

import moments_model as M
from ptmcmc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mean", "cov", "var", "walker_sum", "count")


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def assert_same(got, want, what):
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES, got, want):
        if w is None or g is None:
            assert g is None and w is None, (what, name)
        else:
            assert np.shape(g) == np.shape(w) and same_bits(g, w), (what, name, np.ravel(g)[:4], np.ravel(w)[:4])


@pytest.fixture(scope="module")
def fixture_exe():
    with tempfile.TemporaryDirectory() as d:
        yield M.build_fixture_driver(d)


@pytest.fixture(scope="module")
def sanitized_exe():
    with tempfile.TemporaryDirectory() as d:
        yield M.build_fixture_driver(d, sanitize=True)


def constant_feature_series(n, ns, nf, seed):
    x = M.ar1_series(n, ns, nf, seed)
    x[:, :, nf - 1] = 2.5
    return x


@pytest.mark.parametrize("W", [1, 64, 65, 129])
@pytest.mark.parametrize("nfeat", [1, 3])
def test_the_facade_estimator_and_the_twin_agree_bit_for_bit(fixture_exe, W, nfeat):
    series = M.ar1_series(12, W, nfeat, seed=100 * W + nfeat)
    for nrows in (2, 5, 12):
        for cov in (True, False):
            want = M.moments(M.series_window(series, nrows), cov=cov)
            assert_same(M.fixture_driver_answers(fixture_exe, series, nrows, cov=cov), want, (W, nfeat, nrows, cov))
    if W > 1:
        assert_same(M.fixture_driver_answers(fixture_exe, series, 1), M.moments(M.series_window(series, 1)), (W, nfeat, "one row"))


def test_a_constant_feature_gives_an_exact_zero_row_and_column(fixture_exe):
    series = constant_feature_series(9, 65, 3, seed=5)
    want = M.moments(series)
    assert (want[1][2] == 0).all() and (want[1][:, 2] == 0).all() and want[2][2] == 0 and want[0][2] == 2.5
    assert np.all(np.diagonal(want[1])[:2] > 0)
    assert_same(M.fixture_driver_answers(fixture_exe, series, 9), want, "constant feature")


@pytest.mark.parametrize("shape", [(40, 70, 3), (7, 129, 5), (300, 1, 2), (25, 64, 33)])
def test_twin_agrees_with_numpy_cov(shape):
    """per entry within 4 N eps sum |d_i d_j| / (N - 1), the bound of a sum of N products each rounded once, computed from the data"""
    series = M.ar1_series(*shape, seed=7)
    n, W, nf = shape
    N = n * W
    mean, cov, var, s_w, count = M.moments(series)
    flat = series.reshape(N, nf)
    want = np.cov(flat, rowvar=False).reshape(nf, nf)
    d = flat - flat.mean(axis=0)
    bound = 4 * N * np.finfo(np.float64).eps * (np.abs(d).T @ np.abs(d)) / (N - 1)
    err = np.abs(cov - want)
    print(shape, "max err / bound", (err / bound).max())
    assert count == N and (err <= bound).all()
    assert np.all(np.abs(mean - flat.mean(axis=0)) <= 4 * N * np.finfo(np.float64).eps * np.abs(flat).sum(axis=0) / N)
    assert same_bits(var, np.diagonal(cov)) and same_bits(cov, cov.T)
    assert same_bits(M.moments(series, cov=False)[2], var)          # the variances alone: the diagonal pairs' sums


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptm_engine.h")).read(), flags=re.S)
    lib = C.CDLL(E.LIB_PATH)
    for name in ("ptm_moments", "ptm_moments_series", "ptm_moments_tile_rows"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
        assert name in E.EXPORTS
    assert "#define PTM_ABI_VERSION 3" in txt or lib.ptm_abi_version() == 3
    assert hasattr(E.Engine, "posterior_moments") and callable(E.moments_series)
    assert E.moments_tile_rows(128) >= 2 and E.moments_tile_rows(3) * 3 <= 4096 and E.moments_tile_rows(129) == 0 and E.moments_tile_rows(0) == 0


def test_null_arguments_are_refused_before_a_device_is_touched():
    L = E.load()
    mean, cov = np.full(3, -7.0), np.full((3, 3), -7.0)
    count = C.c_int64(-7)
    x = np.zeros((4, 2, 3))
    assert L.ptm_moments(None, 0, 3, 2, E._d(mean), E._d(cov), None, None, C.byref(count)) == -1
    assert b"null argument" in L.ptm_last_error()
    assert L.ptm_moments_series(-1, E._d(x), 4, 2, 3, 2, None, E._d(cov), None, None, C.byref(count)) == -1
    assert b"null argument" in L.ptm_last_error()
    assert L.ptm_moments_series(-1, None, 4, 2, 3, 2, E._d(mean), E._d(cov), None, None, C.byref(count)) == -1
    assert b"null argument" in L.ptm_last_error()
    # ... and so are the shapes that need no device to be judged
    big = np.zeros((2, 2, 130))
    m130, c130 = np.full(130, -7.0), np.full((130, 130), -7.0)
    assert L.ptm_moments_series(-1, E._d(big), 2, 2, 130, 2, E._d(m130), E._d(c130), None, None, None) == -2      # PTM_ERR_UNSUPPORTED
    assert b"128" in L.ptm_last_error()
    for n, ns, nf, nrows in ((4, 2, 3, 0), (4, 2, 3, 5), (4, 2, 0, 2), (4, 1, 3, 1)):
        assert L.ptm_moments_series(-1, E._d(x), n, ns, nf, nrows, E._d(mean), E._d(cov), None, None, C.byref(count)) == -1, (n, ns, nf, nrows)
    assert (mean == -7).all() and (cov == -7).all() and count.value == -7 and (m130 == -7).all() and (c130 == -7).all()


# ---- the covariance file --------------------------------------------------------------------------------------------------------
def awkward_moments(D=4):
    rng = np.random.default_rng(3)
    a = rng.standard_normal((D, D)) * 10.0 ** rng.integers(-12, 12, size=(D, D))
    cov = a + a.T
    cov[0, 1] = cov[1, 0] = 0.1 + 0.2                               # values that need all 17 digits
    cov[2, 2] = np.nextafter(1.0, 2.0)
    cov[3, 3] = 5e-324
    mean = np.array([1.0 / 3.0, -0.0, 1e308, np.pi])[:D]
    return mean, cov


def check_file_code(exe, d):
    mean, cov = awkward_moments()
    path = os.path.join(d, "moments.cov")
    M.write_file(exe, path, mean, cov, count=140, replicas=70, rows=2, names=["a", "b", "c", "d"])
    head = [ln for ln in open(path) if ln.startswith("#")]
    assert "dim 4" in head[0] and "N 140" in head[0] and "replicas 70 x rows 2" in head[0] and head[1].split()[-4:] == ["a", "b", "c", "d"]
    rc, m2, c2, _ = M.read_file(exe, path, 4)
    assert rc == 0 and same_bits(m2, mean) and same_bits(c2, cov)
    pm, pc = M.parse_file(path)
    assert same_bits(pm, mean) and same_bits(pc, cov)
    text = open(path).read()
    rows = text.strip().splitlines()
    bad = {
        "wrong dimension": (text, 3),
        "missing file": (None, 4),
        "not symmetric": ("\n".join(rows[:-1] + [rows[-1].replace(rows[-1].split()[0], "1.5", 1)]) + "\n", 4),
        "not finite": (text.replace(rows[3].split()[0], "nan", 1), 4),
        "infinite": (text.replace(rows[3].split()[0], "inf", 1), 4),
        "a row short": ("\n".join(rows[:-1]) + "\n", 4),
        "a value short": ("\n".join(rows[:-1] + [" ".join(rows[-1].split()[:-1])]) + "\n", 4),
        "not a number": (text.replace(rows[3].split()[1], "abc", 1), 4),
        "empty": ("# nothing\n", 4),
    }
    for what, (body, dim) in bad.items():
        p = os.path.join(d, "bad.cov")
        if os.path.exists(p):
            os.remove(p)
        if body is not None:
            open(p, "w").write(body)
        rc, _, _, said = M.read_file(exe, p, dim)
        assert rc == 1 and "read_covariance" in said, (what, rc, said[-300:])


def test_covariance_file_round_trip_and_refusals(fixture_exe):
    with tempfile.TemporaryDirectory() as d:
        check_file_code(fixture_exe, d)


def test_estimator_and_file_code_under_the_sanitizers(sanitized_exe):
    """the same program built with -fsanitize=address,undefined: a finding ends it with a non-zero status"""
    for W, nf, nrows, cov in ((1, 1, 2, True), (65, 3, 5, True), (129, 2, 1, True), (3, 130, 4, False), (64, 33, 3, True)):
        series = M.ar1_series(6, W, nf, seed=W + nf)
        assert_same(M.fixture_driver_answers(sanitized_exe, series, nrows, cov=cov), M.moments(M.series_window(series, nrows), cov=cov), (W, nf, nrows, cov))
    with tempfile.TemporaryDirectory() as d:
        check_file_code(sanitized_exe, d)
