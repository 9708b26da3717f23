"""The facade's rhat_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) restated line by line in Python, the checker of the device's split
R-hat kernels (ptm_rhat, ptm_rhat_series; the definition stands in include/ptm_engine.h).

Every floating-point operation is the C++ one, in its order: the sums over a sequence's rows and over the sequences run
sequentially (np.add.accumulate, which adds one element after the other -- never np.sum, which adds pairwise); everything else is
elementwise float64 arithmetic over the lanes (a lane per sequence and feature, then a lane per feature).
"""
import numpy as np


def _seq_sum(t):
    """0.0 + t[0] + t[1] + ... from the left along axis 0"""
    t = np.asarray(t, dtype=np.float64)
    return np.add.accumulate(np.concatenate([np.zeros((1,) + t.shape[1:]), t]), axis=0)[-1]


def split(window):
    """window [nrows, W, nfeat] in ascending row order -> [n, 2 W, nfeat]: the halves of walker w are sequences 2w and 2w + 1"""
    window = np.asarray(window, dtype=np.float64)
    nrows, W, nf = window.shape
    assert nrows >= 4 and nrows % 2 == 0
    n = nrows // 2
    return np.ascontiguousarray(window.reshape(2, n, W, nf).transpose(1, 2, 0, 3).reshape(n, 2 * W, nf))


def sequences(window):
    """(seq_mean, seq_var)[2 W, nfeat]: two walks over each sequence's rows"""
    x = split(window)
    n = x.shape[0]
    with np.errstate(all="ignore"):
        mean = _seq_sum(x) / float(n)
        d = x - mean
        var = _seq_sum(d * d) / float(n - 1)
    return mean, var


def combine(seq_mean, seq_var, n):
    """(rhat, M, within, between)[nfeat] of m sequences of n rows each, sequentially over k = 0 .. m - 1"""
    m = seq_mean.shape[0]
    nd, md = float(n), float(m)
    with np.errstate(all="ignore"):
        M = _seq_sum(seq_mean) / md
        d = seq_mean - M
        between = nd * _seq_sum(d * d) / (md - 1.0)
        within = _seq_sum(seq_var) / md
        var_plus = ((nd - 1.0) / nd) * within + between / nd
        rhat = np.sqrt(var_plus / within)
    return rhat, M, within, between


def split_rhat(window, detail=False):
    """(rhat, mean, within, between)[nfeat] of window [nrows, W, nfeat]; detail=True adds (seq_mean, seq_var)"""
    seq_mean, seq_var = sequences(window)
    out = combine(seq_mean, seq_var, window.shape[0] // 2)
    return out + (seq_mean, seq_var) if detail else out


def series_window(series, nrows):
    """the newest nrows rows of series [n, nseries, nfeat]"""
    series = np.asarray(series, dtype=np.float64)
    return series[series.shape[0] - nrows:]


def ring_window(hist, chains, add_every_n, nhist, nrows):
    """(complete, window[nrows, len(chains), dim]) from Engine.history(): chain c's window is its own newest nrows saved rows,
    newest = 1 + (nhist - 1) // add_every_n, saved row r in slot r % capacity if the slot still holds that row"""
    chains = np.arange(hist["row"].shape[1])[chains]
    nhist = np.asarray(nhist, dtype=np.int64)
    cap = hist["x"].shape[0]
    newest = 1 + (nhist - 1) // add_every_n
    rows = newest[None, :] - nrows + 1 + np.arange(nrows, dtype=np.int64)[:, None]
    assert rows.min() >= 1                                  # row 0, the start state, is never part of a window
    slot = rows % cap
    there = hist["row"][slot, chains[None, :]] == rows
    return bool(there.all()), np.ascontiguousarray(hist["x"][slot, chains[None, :]])


def textbook(window):
    """(rhat, mean, within, between) by the vectorised textbook evaluation over the split sequences"""
    x = split(window)
    n, m = x.shape[0], x.shape[1]
    means, variances = np.mean(x, axis=0), np.var(x, axis=0, ddof=1)
    within = np.mean(variances, axis=0)
    between = n * np.var(means, axis=0, ddof=1)
    var_plus = (n - 1.0) / n * within + between / n
    return np.sqrt(var_plus / within), np.mean(means, axis=0), within, between


def equal_sequences(W=6):
    """window [10, W, 2] in which every half of every walker holds the same rows: small integers (every sum is exact) of mean 3 and
    variance 2 and 8 (powers of two: (n - 1) / n * within / within is exact), so between == 0 and rhat == sqrt((n - 1) / n) to the bit"""
    half = np.array([[5.0, 3.0], [1.0, 7.0], [3.0, -1.0], [3.0, 3.0], [3.0, 3.0]])[:, None, :]
    return np.tile(np.concatenate([half, half]), (1, W, 1))


def two_groups(W=40, nrows=200, nf=2):
    """window of two groups of walkers whose means differ by 10 within-sigma: var_plus ~ within * (1 + 25), rhat about 5"""
    rng = np.random.default_rng(4)
    x = rng.standard_normal((nrows, W, nf))
    x[:, W // 2:] += 10.0
    return x


def build_fixture_driver(d):
    """tests/cxx/rhat_fixture_main.cc: the facade's rhat_estimator on series piped to it (no engine, no library)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(d, "rhat_fx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "ptmcmc_amd", "host"),
                           os.path.join(root, "tests", "cxx", "rhat_fixture_main.cc"), "-L", os.path.join(root, "ptmcmc_amd"), "-lptm_engine",
                           "-Wl,-rpath," + os.path.join(root, "ptmcmc_amd"), "-pthread", "-o", exe])
    return exe


def fixture_driver_answers(exe, series, nrows):
    """(rhat, mean, within, between, seq_mean, seq_var) of the fixture program for series [n, nseries, nfeat] (%.17g round-trips a double)"""
    import subprocess
    series = np.asarray(series, dtype=np.float64)
    n, ns, nf = series.shape
    lines = ["%d %d %d %d" % (n, ns, nf, nrows)] + [" ".join("%.17g" % v for v in row) for row in series.reshape(n, ns * nf)]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    feat = np.array([[float(v) for v in r[1:]] for r in rows if r[0] == "feature"]).reshape(nf, 4)
    seq = np.array([[float(v) for v in r[1:]] for r in rows if r[0] == "sequence"]).reshape(2 * ns, nf, 2)
    return feat[:, 0], feat[:, 1], feat[:, 2], feat[:, 3], seq[..., 0], seq[..., 1]
