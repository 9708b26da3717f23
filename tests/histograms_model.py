"""The facade's histogram_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) restated in Python, the checker of the device's corner-plot
histograms (ptm_histograms, ptm_histograms_series; the definition stands in include/ptm_engine.h).

The edges of feature f are  lo + float(k) * ((hi - lo) / float(nbins))  for k < nbins and hi itself for k = nbins, formed with
Python floats (one rounding per operation, nothing fused): np.linspace(lo, hi, nbins + 1) bit for bit.  x lies in bin
np.searchsorted(edges, x, 'right') - 1, the last bin closed (x == hi: bin nbins - 1); x < lo counts as below, x > hi as above, a NaN
as neither.  Pairs i < j in row-major order: p = i * nfeat - i * (i + 1) / 2 + (j - i - 1).
"""
import numpy as np

OUTSIDE = -1


def edges(lo, hi, nbins):
    """the nbins + 1 edges of one feature, Python floats"""
    lo, hi = float(lo), float(hi)
    step = (hi - lo) / float(nbins)
    return np.array([lo + float(k) * step for k in range(nbins)] + [hi], dtype=np.float64)


def edges_ok(lo, hi, nbins):
    """the definition's own condition: finite, lo < hi, strictly increasing edges"""
    with np.errstate(over="ignore", invalid="ignore"):
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            return False
        e = edges(lo, hi, nbins)
    return bool(np.isfinite(e).all() and (np.diff(e) > 0).all())


def bins(x, lo, hi, nbins):
    """(bin index of every x or OUTSIDE, below, above): one feature"""
    x = np.asarray(x, dtype=np.float64)
    e = edges(lo, hi, nbins)
    k = np.searchsorted(e, x, "right") - 1
    k = np.where(x == e[nbins], nbins - 1, k)                        # the last bin is closed
    with np.errstate(invalid="ignore"):
        below, above = x < e[0], x > e[nbins]
    inside = ~(below | above | np.isnan(x))
    return np.where(inside, k, OUTSIDE), int(below.sum()), int(above.sum())


def pair_index(nfeat, i, j):
    assert 0 <= i < j < nfeat
    return i * nfeat - i * (i + 1) // 2 + (j - i - 1)


def pairs(nfeat):
    return [(i, j) for i in range(nfeat) for j in range(i + 1, nfeat)]


def histograms(window, lo, hi, nbins, with_pairs=True):
    """(h1[nfeat, nbins], h2[npairs, nbins, nbins] or None, below, above, N) of window [nrows, W, nfeat], int64"""
    window = np.asarray(window, dtype=np.float64)
    nf = window.shape[-1]
    x = window.reshape(-1, nf)
    N = x.shape[0]
    h1 = np.zeros((nf, nbins), dtype=np.int64)
    below, above = np.zeros(nf, dtype=np.int64), np.zeros(nf, dtype=np.int64)
    k = np.empty((N, nf), dtype=np.int64)
    for f in range(nf):
        k[:, f], below[f], above[f] = bins(x[:, f], lo[f], hi[f], nbins)
        h1[f] = np.bincount(k[k[:, f] >= 0, f], minlength=nbins)
    h2 = None
    if with_pairs:
        h2 = np.zeros((nf * (nf - 1) // 2, nbins, nbins), dtype=np.int64)
        for i, j in pairs(nf):
            both = (k[:, i] >= 0) & (k[:, j] >= 0)
            flat = np.bincount(k[both, i] * nbins + k[both, j], minlength=nbins * nbins)
            h2[pair_index(nf, i, j)] = flat.reshape(nbins, nbins)
    return h1, h2, below, above, N


def series_window(series, nrows):
    """the newest nrows rows of series [n, nseries, nfeat]"""
    series = np.asarray(series, dtype=np.float64)
    return series[series.shape[0] - nrows:]


def ulps_wide_range(width=300):
    """a range `width` ulps wide at 1.0: the guess of a bin from one multiply is worthless there"""
    return 1.0, 1.0 + width * 2.0 ** -52


def adversarial(lo, hi, nbins, filler=200, seed=0):
    """the values at which a binning goes wrong: every edge, both neighbours of every edge in the doubles, lo, hi, +-0, +-inf,
    values far outside the range, and a uniform filler over a little more than the range"""
    rng = np.random.default_rng(seed)
    e = edges(lo, hi, nbins)
    width = hi - lo
    far = [lo - 1e3 * width, hi + 1e3 * width, -1e300, 1e300, lo - width, hi + width]
    v = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), [lo, hi, 0.0, -0.0, np.inf, -np.inf], far,
                        rng.uniform(lo - 0.1 * width, hi + 0.1 * width, filler)])
    return rng.permutation(v)


def adversarial_series(ranges, nbins, nseries, seed=0, filler=200):
    """series [n, nseries, nfeat] whose feature f holds adversarial(*ranges[f]) (cycled to a common length), and the n"""
    cols = [adversarial(lo, hi, nbins, filler, seed + f) for f, (lo, hi) in enumerate(ranges)]
    n = -(-max(c.size for c in cols) // nseries)
    x = np.stack([np.resize(c, n * nseries) for c in cols], axis=1)
    return x.reshape(n, nseries, len(ranges))


def build_fixture_driver(d, sanitize=False):
    """tests/cxx/histograms_main.cc: the facade's histogram_estimator, the corner file's writer / reader and the sampler's flag
    parsing on data piped to them (no device).  sanitize: built with the address and undefined-behaviour sanitizers (a stand-alone
    host program)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(d, "histograms_fx_san" if sanitize else "histograms_fx")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++11"] + flags + ["-ffp-contract=off", "-Wall", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "ptmcmc_amd", "host"),
                           os.path.join(root, "tests", "cxx", "histograms_main.cc"), "-pthread", "-o", exe])
    return exe


def _ints(text, tag):
    return [[int(v) for v in ln.split()[1:]] for ln in text.strip().splitlines() if ln.split()[0] == tag]


def fixture_driver_answers(exe, series, nrows, lo, hi, nbins, with_pairs=True):
    """(h1, h2, below, above, N) of the fixture program for series [n, nseries, nfeat]; a refusal: (returncode, text)"""
    import subprocess
    series = np.asarray(series, dtype=np.float64)
    n, ns, nf = series.shape
    lines = ["%d %d %d %d %d %d" % (n, ns, nf, nrows, nbins, 1 if with_pairs else 0), " ".join("%.17g" % v for v in lo), " ".join("%.17g" % v for v in hi)]
    lines += [" ".join("%.17g" % v for v in row) for row in series.reshape(n, ns * nf)]
    out = subprocess.run([exe, "estimate"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    if out.returncode:
        return out.returncode, out.stdout + out.stderr
    t = out.stdout
    h1 = np.array(_ints(t, "h1"), dtype=np.int64).reshape(nf, nbins)
    h2 = np.array(_ints(t, "h2"), dtype=np.int64).reshape(nf * (nf - 1) // 2, nbins, nbins) if with_pairs else None
    return h1, h2, np.array(_ints(t, "below")[0], dtype=np.int64), np.array(_ints(t, "above")[0], dtype=np.int64), _ints(t, "count")[0][0]
