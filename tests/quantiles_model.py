"""The facade's quantile_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh) restated in Python, the checker of the device's exact posterior
quantiles (ptm_quantiles, ptm_quantiles_series; the definition stands in include/ptm_engine.h).

The sample of a feature is ordered by the 64-bit key  u ^ (u >> 63 ? ~0 : 1 << 63)  of its values' bit patterns (np.sort on the
keys); the quantile of a probability p is  h = float(N - 1) * p, lo = floor(h), hi = min(lo + 1, N - 1), g = h - lo,
q = s_lo if g == 0 else s_lo + g * (s_hi - s_lo): every operation the C++ one, in float64.
"""
import numpy as np

TOP = np.uint64(1) << np.uint64(63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys(x):
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where((u >> np.uint64(63)) != 0, u ^ ALL, u ^ TOP)


def values(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where((k >> np.uint64(63)) != 0, k ^ TOP, k ^ ALL).view(np.float64)


def ranks(N, p):
    """(lo, hi, g) of probability p in a sample of N"""
    h = float(N - 1) * float(p)
    fl = float(np.floor(h))
    lo = int(fl)
    return lo, min(lo + 1, N - 1), h - fl


def quantiles(window, probs):
    """(q[nq, nfeat], x_lo, x_hi, N) of window [nrows, W, nfeat]: the sample of a feature is every value of the window"""
    window = np.asarray(window, dtype=np.float64)
    nf = window.shape[-1]
    s = values(np.sort(keys(window.reshape(-1, nf)), axis=0))        # [N, nfeat], every column sorted by key
    N = s.shape[0]
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    q, x_lo, x_hi = (np.empty((probs.size, nf)) for _ in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        for k, p in enumerate(probs):
            lo, hi, g = ranks(N, p)
            a, c = s[lo], s[hi]
            q[k] = a if g == 0 else a + np.float64(g) * (c - a)
            x_lo[k], x_hi[k] = a, c
    return q, x_lo, x_hi, N


def series_window(series, nrows):
    """the newest nrows rows of series [n, nseries, nfeat]"""
    series = np.asarray(series, dtype=np.float64)
    return series[series.shape[0] - nrows:]


def skewed_series(n, ns, nf, seed):
    """series [n, ns, nf] with skewed and two-humped marginals around a different level per feature"""
    rng = np.random.default_rng(seed)
    x = np.exp(rng.standard_normal((n, ns, nf)))
    x[..., 1::2] = rng.standard_normal((n, ns, nf))[..., 1::2] + 6.0 * rng.integers(0, 2, size=(n, ns, nf))[..., 1::2]
    return x + np.arange(nf) * 7.0 - 10.0


def build_fixture_driver(d, sanitize=False):
    """tests/cxx/quantiles_main.cc: the facade's quantile_estimator and quantile file writer / reader on data piped to them (no
    device).  sanitize: built with the address and undefined-behaviour sanitizers (a stand-alone host program)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(d, "quantiles_fx_san" if sanitize else "quantiles_fx")
    # (the program uses nothing of the engine: it links without the library; the sanitizers' runtimes are linked in)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++11"] + flags + ["-ffp-contract=off", "-Wall", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "ptmcmc_amd", "host"),
                           os.path.join(root, "tests", "cxx", "quantiles_main.cc"), "-pthread", "-o", exe])
    return exe


def _rows(text, tag):
    return [[float(v) for v in ln.split()[1:]] for ln in text.strip().splitlines() if ln.split()[0] == tag]


def fixture_driver_answers(exe, series, nrows, probs):
    """(q, x_lo, x_hi, N) of the fixture program for series [n, nseries, nfeat] (%.17g round-trips a double)"""
    import subprocess
    series = np.asarray(series, dtype=np.float64)
    n, ns, nf = series.shape
    lines = ["%d %d %d %d %d" % (n, ns, nf, nrows, len(probs)), " ".join("%.17g" % p for p in probs)]
    lines += [" ".join("%.17g" % v for v in row) for row in series.reshape(n, ns * nf)]
    out = subprocess.run([exe, "estimate"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    t = out.stdout
    return np.array(_rows(t, "q")), np.array(_rows(t, "lo")), np.array(_rows(t, "hi")), int(_rows(t, "count")[0][0])


def write_file(exe, path, probs, q, count=0, replicas=0, rows=0, names=None):
    """write_quantiles through the fixture program: (returncode, stdout + stderr)"""
    import subprocess
    q = np.asarray(q, dtype=np.float64)
    nq, D = q.shape
    names = names or ["p%d" % i for i in range(D)]
    text = "%d %d %d %d %d\n%s\n%s\n%s\n" % (D, count, replicas, rows, nq, " ".join("%.17g" % p for p in probs), " ".join(names), " ".join("%.17g" % v for v in q.ravel()))
    out = subprocess.run([exe, "write", path], input=text, capture_output=True, text=True, timeout=60)
    return out.returncode, out.stdout + out.stderr


def read_file(exe, path):
    """read_quantiles through the fixture program: (returncode, head (dim, count, replicas, rows), probs, names, q[nq, dim], said)"""
    import subprocess
    out = subprocess.run([exe, "read", path], capture_output=True, text=True, timeout=60)
    if out.returncode:
        return out.returncode, None, None, None, None, out.stdout + out.stderr
    t = out.stdout
    head = tuple(int(v) for v in _rows(t, "head")[0])
    names = [ln.split()[1:] for ln in t.splitlines() if ln.split()[0] == "names"][0]
    return 0, head, np.array(_rows(t, "probs")[0]), names, np.array(_rows(t, "q")), out.stdout + out.stderr


def parse_file(path):
    """(header words, names, q[nq, dim]) of a quantile file, read in Python"""
    lines = [ln for ln in open(path) if ln.strip()]
    body = [ln.split() for ln in lines if not ln.lstrip().startswith("#")]
    return lines[0].split(), [b[0] for b in body], np.array([[float(v) for v in b[1:]] for b in body]).T
