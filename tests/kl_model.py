"""The facade's kl_estimator and kl_verdict (ptmcmc_amd/host/ptmcmc_gpu.hh) restated in Python: the checker of the device's
nearest-neighbour search (ptm_nn_dist2; the definition stands in include/ptm_engine.h), and tests/golden/kl_divergence.json.gz --
what the real reference answered for its proposal-test statistics (test_proposal.hh:350-502) -- with the named wrong readings the
fixture must tell from the right one.

Every floating-point operation is the C++ one, in its order: a pair's sum runs over the dimensions one after the other (elementwise
float64 arithmetic over all pairs at once), the KL sum over the samples one after the other, and the logarithm is the C library's
(math.log: numpy's own vectorised logarithm may round differently)."""
import functools
import gzip
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KFLOOR = 5


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def enforce_wrap(x, xmin, xmax):
    """boundary::enforce of a wrapped dimension (states.cc:18-28)"""
    width = xmax - xmin
    xt = np.fmod(x - xmin, width)
    xt = np.where(xt < 0, xt + width, xt)
    return xmin + xt


def pair_dist2(P, Q, wrapped=None, xmin=None, xmax=None, wrap_alternative=True):
    """state::dist2 of every pair: [nP, nQ]"""
    P, Q = np.atleast_2d(np.asarray(P, dtype=np.float64)), np.atleast_2d(np.asarray(Q, dtype=np.float64))
    acc = np.zeros((P.shape[0], Q.shape[0]))
    with np.errstate(over="ignore"):
        for d in range(P.shape[1]):
            xa, xb = Q[None, :, d], P[:, None, d]
            diff = np.abs(xb - xa)
            if wrapped is not None and wrapped[d] and wrap_alternative:
                halfwrap = (xmax[d] - xmin[d]) / 2
                alt = np.abs(enforce_wrap(xb - halfwrap, xmin[d], xmax[d]) - enforce_wrap(xa - halfwrap, xmin[d], xmax[d]))
                diff = np.where(alt < diff, alt, diff)
            acc = acc + diff * diff
    return acc


def nn_dist2(P, Q=None, wrapped=None, xmin=None, xmax=None, wrap_alternative=True, skip_self=True):
    """one_nnd2 of every point of P in Q; Q None: all_nnd2, the nearest other index of P itself"""
    d2 = pair_dist2(P, P if Q is None else Q, wrapped, xmin, xmax, wrap_alternative)
    if Q is None and skip_self:
        d2[np.arange(d2.shape[0]), np.arange(d2.shape[0])] = np.inf
    return d2.min(axis=1)


def _log(v):
    v = float(v)
    if v != v or v < 0:
        return math.nan
    return -math.inf if v == 0 else (math.inf if v == math.inf else math.log(v))


def combine(r1sqs, s1sqs, dim, M, floor_index=KFLOOR + 1, floor_both=True, n_less=1.0, sign=-1.0):
    """test_proposal.hh:400-421 from the two distance arrays"""
    r, s = np.array(r1sqs, dtype=np.float64), np.array(s1sqs, dtype=np.float64)
    N = float(len(r))
    if len(r) < KFLOOR + 2 or M < 1:
        raise ValueError("needs at least 7 samples of P and 1 of Q")
    floor = np.sort(r)[floor_index]
    r = np.where(r < floor, floor, r)
    if floor_both:
        s = np.where(s < floor, floor, s)
    result = 0.0
    with np.errstate(all="ignore"):
        ratio = r / s
    for v in ratio:
        result = result + sign * _log(v)
    result = result * ((0.5 * float(dim)) / N)
    return result + math.log(int(M) / (N - n_less))


def kl(P, Q, wrapped=None, xmin=None, xmax=None, detail=False, **wrong):
    """KL_divergence(P, Q, approx_nn=false); detail=True adds the two distance arrays.  wrong: one named reading's switches"""
    P, Q = np.atleast_2d(np.asarray(P, dtype=np.float64)), np.atleast_2d(np.asarray(Q, dtype=np.float64))
    search = {k: wrong.pop(k) for k in ("wrap_alternative", "skip_self") if k in wrong}
    r = nn_dist2(P, None, wrapped, xmin, xmax, **search)
    s = nn_dist2(P, Q, wrapped, xmin, xmax, **{k: v for k, v in search.items() if k == "wrap_alternative"})
    value = combine(r, s, P.shape[1], Q.shape[0], **wrong)
    return (value, r, s) if detail else value


# name -> the switches of kl() that make the mistake
WRONG = {
    "floor_at_sorted_index_5": dict(floor_index=KFLOOR),
    "floor_on_one_array_only": dict(floor_both=False),
    "self_not_excluded": dict(skip_self=False),
    "n_in_place_of_n_minus_1": dict(n_less=0.0),
    "sign_of_the_sum": dict(sign=1.0),
    "wrap_alternative_ignored": dict(wrap_alternative=False),
}


def sample_cov(X):
    """(mean[dim], cov[dim, dim]) sequentially in sample order, divided by N - 1 (test_proposal.hh:592-644)"""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    seq = lambda t: np.add.accumulate(np.concatenate([np.zeros((1,) + t.shape[1:]), t]), axis=0)[-1]
    mean = seq(X) / float(N)
    d = X - mean
    return mean, seq(d[:, :, None] * d[:, None, :]) / (float(N) - 1.0)


def invert(a):
    """(inverse, determinant) by the facade's Gauss-Jordan elimination with partial pivoting"""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    inv, det = np.eye(n), 1.0
    for c in range(n):
        piv = c
        for r in range(c + 1, n):
            if abs(a[r, c]) > abs(a[piv, c]):
                piv = r
        if a[piv, c] == 0.0:
            return None, 0.0
        if piv != c:
            a[[piv, c]], inv[[piv, c]] = a[[c, piv]], inv[[c, piv]]
            det = -det
        d = a[c, c]
        det = det * d
        a[c], inv[c] = a[c] / d, inv[c] / d
        for r in range(n):
            f = a[r, c]
            if r != c and f != 0.0:
                a[r], inv[r] = a[r] - f * a[c], inv[r] - f * inv[c]
    return inv, det


def _seq_dot(u, v):
    s = 0.0
    for a, b in zip(u, v):
        s = s + a * b
    return s


def fake_kl(P, Q):
    """fake_KL_divergence(P, Q) (test_proposal.hh:466-502), nQ = len(P) in the unbiasing factor as written there"""
    P, Q = np.atleast_2d(np.asarray(P, dtype=np.float64)), np.atleast_2d(np.asarray(Q, dtype=np.float64))
    dim, nQ = P.shape[1], P.shape[0]
    meanP, covP = sample_cov(P)
    meanQ, covQ = sample_cov(Q)
    factor = (nQ - dim - 2.0) / (nQ - 1.0)
    inv, _ = invert(covQ)
    if inv is None:
        return math.nan
    inv = inv * factor
    prod = np.array([[_seq_dot(covP[i, :], inv[:, j]) for j in range(dim)] for i in range(dim)])
    trace = 0.0
    for i in range(dim):
        trace = trace + prod[i, i]
    result = 0.0 + (-dim + trace)
    _, det = invert(prod / factor)
    result = result + -_log(det)
    dmu = meanP - meanQ
    quad = 0.0
    for i in range(dim):
        quad = quad + dmu[i] * _seq_dot(inv[i, :], dmu)
    result = result + (quad - (dim + trace) / nQ)
    return 0.5 * result


def verdict(diffs, alt):
    """(Ncut, cut_frac, cut, passes) of test_proposal.hh:311-343 for the redraw values and the alt-transformed value"""
    d = np.sort(np.abs(np.asarray(diffs, dtype=np.float64)))
    ntry = len(d)
    ncut = int(math.sqrt(ntry))
    cut = (d[ntry - ncut] + d[ntry - ncut - 1]) / 2.0 if ntry > 1 else 0.0
    return ncut, ncut * 1.0 / ntry, float(cut), bool(alt < cut)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def load():
    with gzip.open(os.path.join(HERE, "golden", "kl_divergence.json.gz"), "rt") as f:
        fx = json.load(f)
    scale = float(fx["coordinate_scale"])
    for c in fx["cases"]:
        c["P"] = np.array(c["P_int"], dtype=np.float64).reshape(-1, c["dim"]) / scale     # exact: integers over a power of two
        c["Q"] = np.array(c["Q_int"], dtype=np.float64).reshape(-1, c["dim"]) / scale
        c["bounds"] = (np.array(c["wrapped"], dtype=np.int32), np.array(c["xmin"], dtype=np.float64), np.array(c["xmax"], dtype=np.float64))
    return fx


def sets_input(cases, head="sets "):
    """the text both programs read (tests/cxx/kl_fixture_main.cc, tests/golden/make_kl_fixture.cc)"""
    lines = ["%s%d" % (head, len(cases))]
    for c in cases:
        P, Q = np.atleast_2d(c["P"]), np.atleast_2d(c["Q"])
        w, lo, hi = c["bounds"]
        lines.append("%d %d %d" % (P.shape[1], P.shape[0], Q.shape[0]))
        lines += ["%d %.17g %.17g" % (w[d], lo[d], hi[d]) for d in range(P.shape[1])]
        lines += [" ".join("%.17g" % v for v in row) for row in P] + [" ".join("%.17g" % v for v in row) for row in Q]
    return "\n".join(lines) + "\n"


def parse_sets_output(text):
    """[{kl, fkl, r, s}] of either program's answers (%.17g round-trips a double)"""
    out = []
    for ln in text.strip().splitlines():
        w = ln.split()
        if w[0] == "kl":
            out.append({})
        out[-1][w[0]] = float(w[1]) if w[0] in ("kl", "fkl") else np.array([float(v) for v in w[1:]])
    return out


def build_fixture_driver(d):
    """tests/cxx/kl_fixture_main.cc: the facade's kl_estimator and kl_verdict on data piped to them (no engine, no device)"""
    import subprocess
    root = os.path.dirname(HERE)
    exe = os.path.join(d, "kl_fx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "ptmcmc_amd", "host"),
                           os.path.join(root, "tests", "cxx", "kl_fixture_main.cc"), "-L", os.path.join(root, "ptmcmc_amd"), "-lptm_engine",
                           "-Wl,-rpath," + os.path.join(root, "ptmcmc_amd"), "-pthread", "-o", exe])
    return exe


def run_driver(exe, text):
    import subprocess
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout
