"""Corner-plot histograms without a device: the Python twin (tests/histograms_model.py) of the facade's histogram_estimator against
np.histogram / np.histogram2d and against the facade itself (tests/cxx/histograms_main.cc, every integer); the refusal of ranges
that cannot hold their bins; the C ABI's declarations, exports and early refusals; the corner file's round trip and refusals; the
sampler's corner flags; and the estimator and the file code under the address and undefined-behaviour sanitizers (a stand-alone host
program)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import histograms_model as H
from ptmcmc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("h1", "h2", "below", "above", "count")
NBINS = [1, 2, 20, 127, 128]
RANGES = [(-3.0, 5.0), (0.0, 1.0), (-1e5, 1e5), (1e300, 3e300), (-2e-300, 5e-300), (2.5e-6, 2.5e-6 + 1e-9), (1e-5, 3e-5), (-7.0, 0.0), H.ulps_wide_range()]


def assert_same(got, want, what):
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, (what, name)
            continue
        assert np.shape(g) == np.shape(w) and np.array_equal(g, w), (what, name)


@pytest.fixture(scope="module")
def fixture_exe():
    with tempfile.TemporaryDirectory() as d:
        yield H.build_fixture_driver(d)


@pytest.fixture(scope="module")
def sanitized_exe():
    with tempfile.TemporaryDirectory() as d:
        yield H.build_fixture_driver(d, sanitize=True)


# ---- the twin against numpy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins", NBINS)
def test_the_edges_are_numpys_linspace_and_the_engines(nbins):
    for lo, hi in RANGES:
        e = H.edges(lo, hi, nbins)
        assert e.tobytes() == np.linspace(lo, hi, nbins + 1).tobytes(), (lo, hi)
        assert e.tobytes() == E.histogram_edges(lo, hi, nbins).tobytes()
    both = E.histogram_edges([r[0] for r in RANGES], [r[1] for r in RANGES], nbins)
    assert both.shape == (len(RANGES), nbins + 1) and all(both[i].tobytes() == H.edges(*RANGES[i], nbins).tobytes() for i in range(len(RANGES)))


@pytest.mark.parametrize("nbins", NBINS)
def test_twin_counts_are_numpys(nbins):
    """every edge, both its neighbours in the doubles, lo, hi, +-0, +-inf, far values: np.histogram counts them as the definition does
    (values outside the range dropped; numpy takes no infinities in the data, they are counted here as below and above)"""
    for r, (lo, hi) in enumerate(RANGES):
        if not H.edges_ok(lo, hi, nbins):
            assert (lo, hi) == H.ulps_wide_range() and nbins > 100 or hi - lo == 0, (lo, hi, nbins)
            continue
        x = H.adversarial(lo, hi, nbins, seed=r)
        k, below, above = H.bins(x, lo, hi, nbins)
        finite = x[np.isfinite(x)]
        want = np.histogram(finite, nbins, (lo, hi))[0]
        assert np.array_equal(np.bincount(k[k >= 0], minlength=nbins), want), (lo, hi)
        assert below == (x < lo).sum() and above == (x > hi).sum() and below + above + want.sum() == x.size
        assert below >= 3 and above >= 3 and want[nbins - 1] >= 2                 # -inf, the far values; hi itself lies in the last bin
    assert H.edges_ok(*H.ulps_wide_range(), 20) and H.edges_ok(*H.ulps_wide_range(), 2)


@pytest.mark.parametrize("nbins", [1, 2, 20, 128])
def test_twin_pair_counts_are_numpys(nbins):
    ranges = [RANGES[0], RANGES[1], H.ulps_wide_range(), RANGES[5]]
    x = H.adversarial_series(ranges, nbins, 3, seed=nbins)
    x = x[np.isfinite(x).all(axis=(1, 2))]                          # (np.histogram2d takes no infinities)
    lo, hi = np.array([r[0] for r in ranges]), np.array([r[1] for r in ranges])
    h1, h2, below, above, N = H.histograms(x, lo, hi, nbins)
    flat = x.reshape(-1, len(ranges))
    assert N == flat.shape[0] and h2.shape == (6, nbins, nbins)
    for i, j in H.pairs(len(ranges)):
        want = np.histogram2d(flat[:, i], flat[:, j], nbins, [(lo[i], hi[i]), (lo[j], hi[j])])[0]
        assert np.array_equal(h2[H.pair_index(len(ranges), i, j)], want.astype(np.int64)), (i, j)
    assert [H.pair_index(4, i, j) for i, j in H.pairs(4)] == list(range(6))
    for f in range(len(ranges)):
        assert np.array_equal(h1[f], np.histogram(flat[:, f], nbins, (lo[f], hi[f]))[0])


def test_ranges_that_cannot_hold_their_bins_are_refused_where_numpy_refuses():
    lo, hi = H.ulps_wide_range(3)
    assert not H.edges_ok(lo, hi, 4) and H.edges_ok(lo, hi, 3) and H.edges_ok(lo, hi, 1)
    with pytest.raises(ValueError):
        np.histogram(np.array([lo]), 4, (lo, hi))
    assert np.histogram(np.array([lo, hi]), 3, (lo, hi))[0].tolist() == [1, 0, 1]
    for a, b in ((1.0, 1.0), (2.0, 1.0), (0.0, np.inf), (np.nan, 1.0), (-1e308, 1e308), (0.0, 5e-324 * 3)):
        assert not H.edges_ok(a, b, 4), (a, b)


# ---- the twin against the facade ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins", NBINS)
def test_the_facade_estimator_and_the_twin_agree_in_every_count(fixture_exe, nbins):
    ranges = [r for r in RANGES if H.edges_ok(r[0], r[1], nbins)][:8]
    series = H.adversarial_series(ranges, nbins, 3, seed=nbins, filler=40)
    lo, hi = [r[0] for r in ranges], [r[1] for r in ranges]
    n = series.shape[0]
    for nrows, pairs in ((n, True), (max(1, n // 3), True), (1, False)):
        want = H.histograms(H.series_window(series, nrows), lo, hi, nbins, pairs)
        assert_same(H.fixture_driver_answers(fixture_exe, series, nrows, lo, hi, nbins, pairs), want, (nbins, nrows, pairs))
    for lo1, hi1 in ranges:
        out = subprocess.run([fixture_exe, "edges"], input="%.17g %.17g %d\n" % (lo1, hi1, nbins), capture_output=True, text=True)
        words = out.stdout.split()
        assert np.array([float(v) for v in words[1:nbins + 2]]).tobytes() == H.edges(lo1, hi1, nbins).tobytes() and words[-2:] == ["ok", "1"]


def test_the_facade_refuses_what_the_twin_refuses(fixture_exe):
    lo, hi = H.ulps_wide_range(3)
    x = np.full((2, 2, 2), 1.0)
    got = H.fixture_driver_answers(fixture_exe, x, 2, [0.0, lo], [2.0, hi], 4)
    assert got[0] == 1 and "refused 1" in got[1]
    assert_same(H.fixture_driver_answers(fixture_exe, x, 2, [0.0, lo], [2.0, hi], 3), H.histograms(x, [0.0, lo], [2.0, hi], 3), "three bins fit")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptm_engine.h")).read(), flags=re.S)
    lib = C.CDLL(E.LIB_PATH)
    for name in ("ptm_histograms", "ptm_histograms_series", "ptm_histograms_last_launch"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
        assert name in E.EXPORTS
    L = E.load()
    assert len(L.ptm_histograms.argtypes) == 12 and len(L.ptm_histograms_series.argtypes) == 14
    assert hasattr(E.Engine, "posterior_histograms") and callable(E.histograms_series) and callable(E.histogram_edges) and callable(E.read_corner)


def test_null_and_bad_arguments_are_refused_before_a_device_is_touched():
    L = E.load()
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    h1, h2 = np.full((3, 4), -7, dtype=np.int64), np.full((3, 4, 4), -7, dtype=np.int64)
    below, above = np.full(3, -7, dtype=np.int64), np.full(3, -7, dtype=np.int64)
    count = C.c_int64(-7)
    x = np.zeros((4, 2, 3))
    lo, hi = np.zeros(3), np.ones(3)
    call = lambda series, n, ns, nf, nrows, nbins, a, b, o1=h1: L.ptm_histograms_series(-1, series, n, ns, nf, nrows, nbins, a, b, i64(o1) if o1 is not None else None,
                                                                                          i64(h2), i64(below), i64(above), C.byref(count))
    assert L.ptm_histograms(None, 0, 3, 2, 4, E._d(lo), E._d(hi), i64(h1), i64(h2), i64(below), i64(above), C.byref(count)) == -1
    assert b"null argument" in L.ptm_last_error()
    for series, a, b, o1 in ((None, E._d(lo), E._d(hi), h1), (E._d(x), None, E._d(hi), h1), (E._d(x), E._d(lo), None, h1), (E._d(x), E._d(lo), E._d(hi), None)):
        assert call(series, 4, 2, 3, 2, 4, a, b, o1) == -1
        assert b"null argument" in L.ptm_last_error()
    for n, ns, nf, nrows, nbins in ((4, 2, 3, 0, 4), (4, 2, 3, 5, 4), (4, 2, 0, 2, 4), (4, 2, 3, 2, 0), (4, 2, 3, 2, 129), (4, 0, 3, 2, 4)):
        assert call(E._d(x), n, ns, nf, nrows, nbins, E._d(lo), E._d(hi)) == -1, (n, ns, nf, nrows, nbins)
    lo_u, hi_u = H.ulps_wide_range(3)
    for a, b, said in (([0, np.nan, 0], [1, 1, 1], b"not finite"), ([0, 1, 0], [1, 1, 1], b"lo < hi"), ([0, 0, 0], [1, np.inf, 1], b"not finite"),
                       ([0, lo_u, 0], [1, hi_u, 1], b"the range cannot hold nbins bins"), ([-1e308, 0, 0], [1e308, 1, 1], b"the range cannot hold nbins bins")):
        a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
        assert call(E._d(x), 4, 2, 3, 2, 4, E._d(a), E._d(b)) == -1 and said in L.ptm_last_error(), (a, b, L.ptm_last_error())
    wide = np.zeros((1, 1, 65))
    assert L.ptm_histograms_series(-1, E._d(wide), 1, 1, 65, 1, 128, E._d(np.zeros(65)), E._d(np.ones(65)), i64(h1), i64(h2), i64(below), i64(above), C.byref(count)) == -2
    assert b"2^25" in L.ptm_last_error()
    xn = x.copy()
    xn[3, 1, 2] = np.nan
    assert call(E._d(xn), 4, 2, 3, 2, 4, E._d(lo), E._d(hi)) == -1
    assert b"NaN" in L.ptm_last_error()
    assert (h1 == -7).all() and (h2 == -7).all() and (below == -7).all() and (above == -7).all() and count.value == -7


def test_there_is_no_cpu_fallback():
    """without a device the call fails and fills nothing: no host path stands in for the kernels"""
    if E.device_count() > 0:
        return
    out = (np.full((3, 4), -7, dtype=np.int64), np.full((3, 4, 4), -7, dtype=np.int64), np.full(3, -7, dtype=np.int64), np.full(3, -7, dtype=np.int64))
    with pytest.raises(E.PtmError):
        E.histograms_series(np.zeros((4, 2, 3)), np.zeros(3) - 1, np.ones(3), 4, out=out)
    assert all((o == -7).all() for o in out)


# ---- the corner file ------------------------------------------------------------------------------------------------------------
def write_file(exe, path, r, names, replicas=70, rows=2, pairs=True):
    h1, h2, below, above, count, lo, hi = r
    D, B = h1.shape
    nums = lambda a: " ".join("%.17g" % v for v in np.ravel(a))
    ints = lambda a: " ".join("%d" % v for v in np.ravel(a))
    text = "%d %d %d %d %d %d\n%s\n%s\n%s\n%s\n%s\n%s\n%s\n" % (D, B, count, replicas, rows, 1 if pairs else 0, " ".join(names), nums(lo), nums(hi), ints(below), ints(above), ints(h1),
                                                              ints(h2) if pairs else "")
    out = subprocess.run([exe, "write", path], input=text, capture_output=True, text=True, timeout=60)
    return out.returncode, out.stdout + out.stderr


def read_file(exe, path):
    out = subprocess.run([exe, "read", path], capture_output=True, text=True, timeout=60)
    return out.returncode, out.stdout + out.stderr


def awkward_counts():
    rng = np.random.default_rng(4)
    D, B = 3, 4
    h1 = rng.integers(0, 1000, (D, B)).astype(np.int64)
    h1[0, 0] = 2 ** 40 + 1                                           # a count that needs 64 bits
    h2 = rng.integers(0, 50, (3, B, B)).astype(np.int64)
    lo = np.array([0.1 + 0.2, -0.0, -1e308])
    hi = np.array([1.0 / 3.0, 5e-324, np.nextafter(-1e308, 0.0)])
    return h1, h2, np.array([0, 5, 2 ** 33], dtype=np.int64), np.array([1, 0, 7], dtype=np.int64), 140, lo, hi


def check_file_code(exe, d):
    r = awkward_counts()
    h1, h2, below, above, count, lo, hi = r
    path = os.path.join(d, "run.corner")
    rc, said = write_file(exe, path, r, ["a", "b", "c"])
    assert rc == 0, said
    assert open(path).readline() == "# posterior histograms: dim 3 nbins 4 N 140 replicas 70 rows 2 pairs 3\n"
    got = E.read_corner(path)                                        # the Python reader
    assert (got["dim"], got["nbins"], got["count"], got["replicas"], got["rows"], got["names"]) == (3, 4, 140, 70, 2, ["a", "b", "c"])
    assert got["lo"].tobytes() == lo.tobytes() and got["hi"].tobytes() == hi.tobytes()
    for name, want in (("h1", h1), ("h2", h2), ("below", below), ("above", above)):
        assert got[name].dtype == np.int64 and np.array_equal(got[name], want), name
    assert got["pairs"] == [("a", "b"), ("a", "c"), ("b", "c")]
    rc, said = read_file(exe, path)                                  # the facade's reader
    assert rc == 0, said
    rows = {}
    for ln in said.splitlines():
        rows.setdefault(ln.split()[0], []).append(ln.split()[1:])
    assert rows["head"] == [["3", "4", "140", "70", "2", "1"]] and rows["names"] == [["a", "b", "c"]]
    assert np.array([float(v) for v in rows["lo"][0]]).tobytes() == lo.tobytes() and np.array([float(v) for v in rows["hi"][0]]).tobytes() == hi.tobytes()
    assert np.array_equal(np.array(rows["h1"], dtype=np.int64), h1) and np.array_equal(np.array(rows["h2"], dtype=np.int64).reshape(3, 4, 4), h2)
    assert np.array_equal(np.array(rows["below"][0], dtype=np.int64), below) and np.array_equal(np.array(rows["above"][0], dtype=np.int64), above)
    # without the pairs: the parameter lines alone
    path1 = os.path.join(d, "one.corner")
    rc, said = write_file(exe, path1, r, ["a", "b", "c"], pairs=False)
    assert rc == 0 and read_file(exe, path1)[0] == 0
    one = E.read_corner(path1)
    assert one["h2"].shape == (0, 4, 4) and np.array_equal(one["h1"], h1)
    rc, said = write_file(exe, os.path.join(d, "bad_name.corner"), r, ["a", "b#", "c"])
    assert rc == 1 and "write_corner" in said
    text = open(path).read()
    lines = text.strip().splitlines()
    bad = {
        "missing file": None,
        "no header": "\n".join(lines[1:]) + "\n",
        "malformed header": text.replace("replicas", "copies", 1),
        "too many bins": text.replace("nbins 4", "nbins 129", 1),
        "other pairs": text.replace("pairs 3", "pairs 2", 1),
        "a line short": "\n".join(lines[:-1]) + "\n",
        "a line more": text + "a b" + " 1" * 16 + "\n",
        "a value short": "\n".join(lines[:-1] + [" ".join(lines[-1].split()[:-1])]) + "\n",
        "a value more": "\n".join(lines[:2] + [lines[2] + " 4"] + lines[3:]) + "\n",
        "not a count": text.replace(" %d " % h1[1, 1], " 1.5 ", 1),
        "a negative count": text.replace(" %d " % h1[1, 1], " -3 ", 1),
        "not a number": text.replace(lines[1].split()[1], "abc", 1),
        "an infinite end": text.replace(lines[1].split()[1], "-inf", 1),
        "an unordered range": text.replace(lines[1].split()[1], "0.5", 1),
        "empty": "",
    }
    for what, body in bad.items():
        p = os.path.join(d, "bad.corner")
        if os.path.exists(p):
            os.remove(p)
        if body is not None:
            assert body != text, what
            open(p, "w").write(body)
        rc, said = read_file(exe, p)
        assert rc == 1 and "read_corner" in said, (what, rc, said[-300:])


def test_corner_file_round_trip_and_refusals(fixture_exe):
    with tempfile.TemporaryDirectory() as d:
        check_file_code(fixture_exe, d)


def test_sampler_flags_and_the_widening_of_an_equal_range(fixture_exe):
    def flags(*a):
        out = subprocess.run([fixture_exe, "flags"] + list(a), capture_output=True, text=True, timeout=60)
        return out.returncode, {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines() if ln and ln.split()[0] in ("bins", "range", "probs", "ends")}, out.stdout
    rc, got, _ = flags("20", "1", "-1.5", "2")
    assert rc == 0 and got == {"bins": ["20"], "range": ["1"], "probs": ["0", "1"], "ends": ["-1.5", "2"]}
    rc, got, _ = flags("128", "0.9", "3", "3")
    assert rc == 0 and got["bins"] == ["128"] and [float(v) for v in got["ends"]] == [2.5, 3.5]               # numpy's rule for an empty range
    assert [float(v) for v in got["probs"]] == [(1.0 - 0.9) / 2.0, (1.0 + 0.9) / 2.0]
    assert np.histogram(np.array([3.0, 3.0]), 4)[1][[0, -1]].tolist() == [2.5, 3.5]
    rc, got, _ = flags("1", "1e-3", "0", "-0.0")
    assert rc == 0 and [float(v) for v in got["ends"]] == [-0.5, 0.5]
    for bins, c in (("0", "1"), ("129", "1"), ("-4", "1"), ("abc", "1"), ("2.5", "1"), ("", "1")):
        rc, _, said = flags(bins, c, "0", "1")
        assert rc == 1 and "--corner_bins" in said, (bins, said)
    for bins, c in (("20", "0"), ("20", "1.5"), ("20", "-0.2"), ("20", "nan"), ("20", "x"), ("20", "")):
        rc, _, said = flags(bins, c, "0", "1")
        assert rc == 1 and "--corner_range" in said, (c, said)


def test_estimator_and_file_code_under_the_sanitizers(sanitized_exe):
    """the same program built with -fsanitize=address,undefined: a finding ends it with a non-zero status"""
    for nbins, ns in ((1, 1), (20, 3), (128, 65), (127, 2)):
        ranges = [r for r in RANGES if H.edges_ok(r[0], r[1], nbins)][:5]
        series = H.adversarial_series(ranges, nbins, ns, seed=nbins + ns, filler=30)
        lo, hi = [r[0] for r in ranges], [r[1] for r in ranges]
        for nrows, pairs in ((series.shape[0], True), (1, False)):
            assert_same(H.fixture_driver_answers(sanitized_exe, series, nrows, lo, hi, nbins, pairs), H.histograms(H.series_window(series, nrows), lo, hi, nbins, pairs), (nbins, ns, nrows))
    with tempfile.TemporaryDirectory() as d:
        check_file_code(sanitized_exe, d)
    out = subprocess.run([sanitized_exe, "flags", "20", "0.5", "1", "1"], capture_output=True, text=True)
    assert out.returncode == 0 and "ends 0.5 1.5" in out.stdout
