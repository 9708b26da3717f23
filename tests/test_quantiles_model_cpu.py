"""Exact posterior quantiles without a device: the Python twin (tests/quantiles_model.py) of the facade's quantile_estimator against
the facade itself (tests/cxx/quantiles_main.cc, bit for bit) and against np.sort / np.quantile; the C ABI's declarations, exports
and early refusals; the quantile file's round trip and refusals; and the estimator and the file code under the address and
undefined-behaviour sanitizers (a stand-alone host program)."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest

import quantiles_model as Q
from ptmcmc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("q", "x_lo", "x_hi", "count")
PROBS = [0.05, 0.5, 0.95, 0.0, 1.0, 0.5, 1e-12, 1.0 / 3.0]


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def assert_same(got, want, what):
    assert len(got) == len(want) == 4
    for name, g, w in zip(NAMES, got, want):
        assert np.shape(g) == np.shape(w) and same_bits(g, w), (what, name, np.ravel(g)[:4], np.ravel(w)[:4])


@pytest.fixture(scope="module")
def fixture_exe():
    with tempfile.TemporaryDirectory() as d:
        yield Q.build_fixture_driver(d)


@pytest.fixture(scope="module")
def sanitized_exe():
    with tempfile.TemporaryDirectory() as d:
        yield Q.build_fixture_driver(d, sanitize=True)


def awkward_series(n, ns, nf, seed):
    """skewed series whose first feature holds zeros of both signs, infinities, denormals and huge values"""
    x = Q.skewed_series(n, ns, nf, seed)
    flat = x[..., 0].reshape(-1)
    odd = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1e-300, -1e300, 0.0, -0.0])
    flat[:min(flat.size, odd.size)] = odd[:flat.size]
    x[..., 0] = flat.reshape(x.shape[:-1])
    return x


@pytest.mark.parametrize("W", [1, 64, 65])
@pytest.mark.parametrize("nfeat", [1, 3])
def test_the_facade_estimator_and_the_twin_agree_bit_for_bit(fixture_exe, W, nfeat):
    series = awkward_series(6, W, nfeat, seed=100 * W + nfeat)
    for nrows in (1, 2, 5):
        want = Q.quantiles(Q.series_window(series, nrows), PROBS)
        assert want[3] == W * nrows
        assert_same(Q.fixture_driver_answers(fixture_exe, series, nrows, PROBS), want, (W, nfeat, nrows))


def test_a_single_sample_is_its_own_every_quantile(fixture_exe):
    series = np.array([[[3.25, -0.0]]])
    q, lo, hi, N = Q.quantiles(series, PROBS)
    assert N == 1 and same_bits(q, np.tile([3.25, -0.0], (len(PROBS), 1))) and same_bits(lo, q) and same_bits(hi, q)
    assert_same(Q.fixture_driver_answers(fixture_exe, series, 1, PROBS), (q, lo, hi, N), "N = 1")


def test_the_key_orders_like_the_reals_with_minus_zero_first():
    x = np.array([np.inf, 1.0, 5e-324, 0.0, -0.0, -5e-324, -1.0, -np.inf])
    k = Q.keys(x)
    assert (np.diff(k.astype(object)) < 0).all()                    # strictly descending keys for strictly descending values
    assert same_bits(Q.values(k), x)


def test_twin_agrees_with_numpy():
    """x_lo / x_hi are np.sort(x)[lo] / [hi] exactly; q lies in [x_lo, x_hi] and within 8 * 2^-52 * max(|x_lo|, |x_hi|) of
    np.quantile: numpy's lerp rounds differently from the definition, each form with three roundings of at most half an ulp of at
    most 2 max|x|; over 3000 random samples, N up to 400, the largest error seen was 1.05 of 2^-52 max|x|."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for trial in range(3000):
        N = int(rng.integers(1, 401))
        x = rng.standard_normal(N) * 10.0 ** rng.integers(-3, 4) + rng.standard_normal() * 10.0 ** rng.integers(-3, 4)
        probs = np.concatenate([rng.uniform(0, 1, 3), [0.0, 1.0, 0.5]])
        q, lo, hi, count = Q.quantiles(x.reshape(N, 1, 1), probs)
        s = np.sort(x)
        want = np.quantile(x, probs)
        assert count == N
        for k, p in enumerate(probs):
            a, b, g = Q.ranks(N, p)
            assert lo[k, 0] == s[a] and hi[k, 0] == s[b]
            assert lo[k, 0] <= q[k, 0] <= hi[k, 0]
            unit = 2.0 ** -52 * max(abs(lo[k, 0]), abs(hi[k, 0]))
            err = abs(q[k, 0] - want[k])
            assert err <= 8 * unit, (trial, N, p, q[k, 0], want[k])
            if unit > 0:
                worst = max(worst, err / unit)
    print("largest |q - np.quantile| in units of 2^-52 max|x|:", worst)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptm_engine.h")).read(), flags=re.S)
    lib = C.CDLL(E.LIB_PATH)
    for name in ("ptm_quantiles", "ptm_quantiles_series", "ptm_quantiles_last_path"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
        assert name in E.EXPORTS
    L = E.load()
    assert len(L.ptm_quantiles.argtypes) == 10 and len(L.ptm_quantiles_series.argtypes) == 12
    assert hasattr(E.Engine, "posterior_quantiles") and callable(E.quantiles_series) and callable(E.quantiles_last_path)


def test_null_and_bad_arguments_are_refused_before_a_device_is_touched():
    L = E.load()
    q, lo, hi = (np.full((2, 3), -7.0) for _ in range(3))
    count = C.c_int64(-7)
    x = np.zeros((4, 2, 3))
    p = np.array([0.25, 0.5])
    assert L.ptm_quantiles(None, 0, 3, 2, 2, E._d(p), E._d(q), E._d(lo), E._d(hi), C.byref(count)) == -1
    assert b"null argument" in L.ptm_last_error()
    for series, probs, out in ((None, E._d(p), E._d(q)), (E._d(x), None, E._d(q)), (E._d(x), E._d(p), None)):
        assert L.ptm_quantiles_series(-1, series, 4, 2, 3, 2, 2, probs, out, E._d(lo), E._d(hi), C.byref(count)) == -1
        assert b"null argument" in L.ptm_last_error()
    # ... and so are the shapes, the probabilities and the values that need no device to be judged
    for n, ns, nf, nrows, nq in ((4, 2, 3, 0, 2), (4, 2, 3, 5, 2), (4, 2, 0, 2, 2), (4, 2, 3, 2, 0), (4, 2, 3, 2, 33), (4, 0, 3, 2, 2)):
        p33 = np.full(33, 0.5)
        assert L.ptm_quantiles_series(-1, E._d(x), n, ns, nf, nrows, nq, E._d(p33), E._d(q), E._d(lo), E._d(hi), C.byref(count)) == -1, (n, ns, nf, nrows, nq)
    for bad in (-1e-9, 1.0000001, np.nan, np.inf):
        pb = np.array([0.5, bad])
        assert L.ptm_quantiles_series(-1, E._d(x), 4, 2, 3, 2, 2, E._d(pb), E._d(q), E._d(lo), E._d(hi), C.byref(count)) == -1, bad
        assert b"[0, 1]" in L.ptm_last_error()
    xn = x.copy()
    xn[3, 1, 2] = np.nan
    assert L.ptm_quantiles_series(-1, E._d(xn), 4, 2, 3, 2, 2, E._d(p), E._d(q), E._d(lo), E._d(hi), C.byref(count)) == -1
    assert b"NaN" in L.ptm_last_error()
    assert (q == -7).all() and (lo == -7).all() and (hi == -7).all() and count.value == -7


def test_there_is_no_cpu_fallback():
    """without a device the call fails and fills nothing: no host path stands in for the kernels"""
    if E.device_count() > 0:
        return
    out = (np.full((1, 3), -7.0),)
    with pytest.raises(E.PtmError):
        E.quantiles_series(np.zeros((4, 2, 3)), [0.5], out=out)
    assert (out[0] == -7).all()


# ---- the quantile file ----------------------------------------------------------------------------------------------------------
def awkward_quantiles():
    q = np.array([[1.0 / 3.0, -0.0, -np.inf, 5e-324],
                  [0.1 + 0.2, 0.0, 1e308, np.nextafter(1.0, 2.0)],
                  [np.pi, 7.0, np.inf, 2.0]])
    return [0.05, 0.5, 1.0 - 2.0 ** -53], q


def check_file_code(exe, d):
    probs, q = awkward_quantiles()
    path = os.path.join(d, "run.quantiles")
    rc, said = Q.write_file(exe, path, probs, q, count=140, replicas=70, rows=2, names=["a", "b", "c", "d"])
    assert rc == 0, said
    head = open(path).readline()
    assert "dim 4" in head and "N 140" in head and "replicas 70 x rows 2" in head and head.split()[-4:-1] == ["probs", "0.050000000000000003", "0.5"]
    rc, h, p2, names, q2, _ = Q.read_file(exe, path)
    assert rc == 0 and h == (4, 140, 70, 2) and same_bits(p2, probs) and names == ["a", "b", "c", "d"] and same_bits(q2, q)
    words, pnames, pq = Q.parse_file(path)
    assert pnames == ["a", "b", "c", "d"] and same_bits(pq, q)
    rc, said = Q.write_file(exe, os.path.join(d, "bad_name.quantiles"), probs, q, names=["a", "b#", "c", "d"])
    assert rc == 1 and "write_quantiles" in said
    text = open(path).read()
    rows = text.strip().splitlines()
    bad = {
        "missing file": None,
        "no header": "\n".join(rows[1:]) + "\n",
        "malformed header": text.replace("replicas", "copies", 1),
        "a probability above 1": text.replace(" 0.5 ", " 1.5 ", 1),
        "no probability": rows[0].split(" probs")[0] + " probs\n" + "\n".join(rows[1:]) + "\n",
        "a line short": "\n".join(rows[:-1]) + "\n",
        "a line more": text + "e 1 2 3\n",
        "a value short": "\n".join(rows[:-1] + [" ".join(rows[-1].split()[:-1])]) + "\n",
        "a value more": "\n".join(rows[:-1] + [rows[-1] + " 4.0"]) + "\n",
        "not a number": text.replace(rows[1].split()[2], "abc", 1),
        "a NaN": text.replace(rows[1].split()[2], "nan", 1),
        "empty": "",
    }
    for what, body in bad.items():
        p = os.path.join(d, "bad.quantiles")
        if os.path.exists(p):
            os.remove(p)
        if body is not None:
            open(p, "w").write(body)
        rc, _, _, _, _, said = Q.read_file(exe, p)
        assert rc == 1 and "read_quantiles" in said, (what, rc, said[-300:])


def test_quantile_file_round_trip_and_refusals(fixture_exe):
    with tempfile.TemporaryDirectory() as d:
        check_file_code(fixture_exe, d)


def test_estimator_and_file_code_under_the_sanitizers(sanitized_exe):
    """the same program built with -fsanitize=address,undefined: a finding ends it with a non-zero status"""
    for W, nf, nrows in ((1, 1, 1), (65, 3, 5), (129, 2, 1), (3, 130, 4), (64, 33, 3)):
        series = awkward_series(6, W, nf, seed=W + nf)
        assert_same(Q.fixture_driver_answers(sanitized_exe, series, nrows, PROBS), Q.quantiles(Q.series_window(series, nrows), PROBS), (W, nf, nrows))
    with tempfile.TemporaryDirectory() as d:
        check_file_code(sanitized_exe, d)
