"""The facade's moments_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) restated in Python, the checker of the device's pooled posterior
moments (ptm_moments, ptm_moments_series; the definition stands in include/ptm_engine.h).

Every floating-point operation is the C++ one, in its order.  The sums whose order matters -- over a walker's rows, over the 64
walkers of a block, over the blocks -- are explicit Python loops that add one term after the other (never np.sum, which adds
pairwise); everything else is elementwise float64 arithmetic over the lanes.
"""
import numpy as np

G = 64          # walkers of a block
COV_MAX = 128   # the device offers the covariance up to this many features


def walker_sums(terms):
    """terms [nrows, W, ...] -> [W, ...]: per walker 0.0 + t[0] + t[1] + ... in row order"""
    s = np.zeros(terms.shape[1:])
    for i in range(terms.shape[0]):
        s = s + terms[i]
    return s


def pooled(per_walker):
    """per_walker [W, ...] -> [...]: the sequential sum over each block's walkers, then the sequential sum over the blocks"""
    W = per_walker.shape[0]
    total = np.zeros(per_walker.shape[1:])
    for b in range(0, W, G):
        block = np.zeros(per_walker.shape[1:])
        for w in range(b, min(b + G, W)):
            block = block + per_walker[w]
        total = total + block
    return total


def moments(window, cov=True):
    """(mean[nfeat], cov[nfeat, nfeat] or None, var[nfeat], walker_sum[W, nfeat], N) of window [nrows, W, nfeat] in ascending row order"""
    window = np.asarray(window, dtype=np.float64)
    nrows, W, nf = window.shape
    N = W * nrows
    assert nrows >= 1 and N >= 2
    s_w = walker_sums(window)
    mean = pooled(s_w) / float(N)
    d = window - mean
    if cov:
        c_w = np.zeros((W, nf, nf))
        for i in range(nrows):                                      # (d_i * d_j == d_j * d_i: both triangles at once)
            c_w = c_w + d[i][:, :, None] * d[i][:, None, :]
        c = pooled(c_w) / float(N - 1)
        return mean, c, np.diagonal(c).copy(), s_w, N
    return mean, None, pooled(walker_sums(d * d)) / float(N - 1), s_w, N


def series_window(series, nrows):
    """the newest nrows rows of series [n, nseries, nfeat]"""
    series = np.asarray(series, dtype=np.float64)
    return series[series.shape[0] - nrows:]


def ar1_series(n, ns, nf, seed):
    """AR(1) series [n, ns, nf] with a different level per feature (tests/test_gpu_rhat.py's)"""
    rng = np.random.default_rng(seed)
    phi = rng.uniform(0.2, 0.95, size=(ns, nf))
    e = rng.standard_normal((n, ns, nf))
    x = np.empty_like(e)
    cur = np.zeros((ns, nf))
    for t in range(n):
        cur = phi * cur + e[t]
        x[t] = cur
    return x + np.arange(nf) * 7.0


def build_fixture_driver(d, sanitize=False):
    """tests/cxx/moments_main.cc: the facade's moments_estimator and covariance file reader / writer on data piped to them (no
    device).  sanitize: built with the address and undefined-behaviour sanitizers (a stand-alone host program)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(d, "moments_fx_san" if sanitize else "moments_fx")
    # (the program uses nothing of the engine: it links without the library; the sanitizers' runtimes are linked in)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++11"] + flags + ["-ffp-contract=off", "-Wall", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "ptmcmc_amd", "host"),
                           os.path.join(root, "tests", "cxx", "moments_main.cc"), "-pthread", "-o", exe])
    return exe


def _rows(text, tag):
    return [[float(v) for v in ln.split()[1:]] for ln in text.strip().splitlines() if ln.split()[0] == tag]


def fixture_driver_answers(exe, series, nrows, cov=True):
    """(mean, cov or None, var, walker_sum, N) of the fixture program for series [n, nseries, nfeat] (%.17g round-trips a double)"""
    import subprocess
    series = np.asarray(series, dtype=np.float64)
    n, ns, nf = series.shape
    lines = ["%d %d %d %d %d" % (n, ns, nf, nrows, 1 if cov else 0)] + [" ".join("%.17g" % v for v in row) for row in series.reshape(n, ns * nf)]
    out = subprocess.run([exe, "estimate"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    t = out.stdout
    c = np.array(_rows(t, "cov")).reshape(nf, nf) if cov else None
    return np.array(_rows(t, "mean")[0]), c, np.array(_rows(t, "var")[0]), np.array(_rows(t, "walker")).reshape(ns, nf), int(_rows(t, "count")[0][0])


def write_file(exe, path, mean, cov, count=0, replicas=0, rows=0, names=None):
    """write_covariance through the fixture program"""
    import subprocess
    mean, cov = np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    D = mean.size
    names = names or ["p%d" % i for i in range(D)]
    text = "%d %d %d %d\n%s\n%s\n%s\n" % (D, count, replicas, rows, " ".join(names), " ".join("%.17g" % v for v in mean), " ".join("%.17g" % v for v in cov.ravel()))
    out = subprocess.run([exe, "write", path], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]


def read_file(exe, path, dim):
    """read_covariance through the fixture program: (returncode, mean, cov, stdout + stderr)"""
    import subprocess
    out = subprocess.run([exe, "read", path, str(dim)], capture_output=True, text=True, timeout=60)
    if out.returncode:
        return out.returncode, None, None, out.stdout + out.stderr
    return 0, np.array(_rows(out.stdout, "mean")[0]), np.array(_rows(out.stdout, "cov")).reshape(dim, dim), out.stdout + out.stderr


def parse_file(path):
    """(mean, cov) of a covariance file, read in Python"""
    rows = [[float(v) for v in ln.split()] for ln in open(path) if ln.strip() and not ln.lstrip().startswith("#")]
    return np.array(rows[0]), np.array(rows[1:])
