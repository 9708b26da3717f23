"""The facade's ess_estimator (ptmcmc_amd/host/ptmcmc_gpu.hh: windowed, report) restated line by line in Python, the checker of the
device's effective-sample-size kernels (ptm_ess_*).

Every floating-point operation is the C++ one, in its order: the per-window sums run sequentially over the samples
(np.add.accumulate, which adds one element after the other -- never np.sum, which adds pairwise); everything behind them is
elementwise float64 arithmetic over the lanes (a lane per series and feature), a lane's `break` being a mask.  A `reader` is the
estimator's validity hook, vectorised: reader(steps) -> (valid[len, nseries], values[len, nseries, nfeat]) for an int array of
nominal steps inside [0, nsteps); steps outside that range are dropped here as ess_estimator::sample does.
"""
import numpy as np


def lag_list(every, burn, per_window):
    lags = [0]
    grow = 1.0
    k = 1
    while k < burn * per_window:
        lags.append(every * k)
        was = k
        while k == was:
            grow *= 1.1
            k = int(grow)
    return lags


def _seq_sum(terms, mask):
    """0.0 + t0 + t1 + ... from the left along axis 0, the terms outside `mask` left out.  A left-out term is added as +0.0: the
    running sum starts at +0.0 and so is never -0.0 (x + y is -0.0 only if both are), and s + 0.0 == s bit for bit for every other s."""
    t = np.where(mask, terms, 0.0)
    return np.add.accumulate(np.concatenate([np.zeros((1,) + t.shape[1:]), t]), axis=0)[-1]


class Estimator:
    """ess_estimator for `nseries` series of `nfeat` features at once (a lane per series and feature, as on the device); the answers
    of windowed() / report() are arrays over the series.  reader(steps) -> (valid[len, nseries], values[len, nseries, >= nfeat])."""

    def __init__(self, steps, nseries, nfeat, reader):
        self.steps, self.nseries, self.nfeat, self.reader = int(steps), int(nseries), int(nfeat), reader

    def sample(self, steps):
        steps = np.asarray(steps, dtype=np.int64)
        inside = (steps >= 0) & (steps < self.steps)
        valid = np.zeros((len(steps), self.nseries), dtype=bool)
        vals = np.zeros((len(steps), self.nseries, self.nfeat))
        if inside.any():
            v, x = self.reader(steps[inside])
            valid[inside] = v
            vals[inside] = np.asarray(x)[:, :, :self.nfeat]
        return valid, vals

    def table(self, width, every, burn):
        """(nwin, lags, mean[w][l][s][f], cov[w][l][s][f], count[w][l][s]) of windowed(), or None where it returns (0, 0) at once"""
        width, every, burn = max(int(width), 2), max(int(every), 1), max(int(burn), 1)
        per_window = width // every
        span = per_window * every
        if per_window < 1:
            return None
        nwin = self.steps // span - burn
        if nwin < 1:
            return None
        origin = self.steps - nwin * span
        lags = lag_list(every, burn, per_window)
        nlag, ns, nf = len(lags), self.nseries, self.nfeat
        mean, cov = np.empty((nwin, nlag, ns, nf)), np.empty((nwin, nlag, ns, nf))
        count = np.empty((nwin, nlag, ns), dtype=np.int64)
        with np.errstate(all="ignore"):
            for w in range(nwin):
                at = origin + w * span + np.arange(per_window, dtype=np.int64) * every
                have, base = self.sample(at)
                for l in range(nlag):
                    if l == 0:
                        m = have
                        s1, s2 = _seq_sum(base, m[..., None]), _seq_sum(base * base, m[..., None])
                    else:
                        ok, then = self.sample(at - lags[l])
                        m = have & ok
                        s1, s2 = _seq_sum(then + base, m[..., None]), _seq_sum(then * base, m[..., None])
                    n = m.sum(axis=0)
                    count[w, l] = n
                    nn = n.astype(np.float64)[:, None]
                    mu = s1 / nn if l == 0 else s1 / nn / 2.0
                    mean[w, l] = mu
                    cov[w, l] = s2 / nn - mu * mu
        return nwin, lags, mean, cov, count

    def feature_ess(self, width, every, burn):
        """e[n - 1][s][f]: feature f's own ess over the newest n windows, n = 1 .. nwin (a feature is a lane of its own: its numbers do
        not depend on which other features are looked at); None where windowed() returns (0, 0) at once"""
        ns, nf = self.nseries, self.nfeat
        t = self.table(width, every, burn)
        if t is None:
            return None
        width, every = max(int(width), 2), max(int(every), 1)
        nwin, lags, mean, cov, count = t
        nlag = len(lags)
        cnt = count.astype(np.float64)[..., None]
        out = np.empty((nwin, ns, nf))
        with np.errstate(all="ignore"):
            for n in range(1, nwin + 1):
                msum = np.zeros((ns, nf))
                for w in range(nwin - n, nwin):
                    msum = msum + mean[w, 0]
                M = msum / float(n)
                length, last_term, previous = np.ones((ns, nf)), np.zeros((ns, nf)), np.ones((ns, nf))
                last_lag = np.zeros((ns, nf))
                going = np.ones((ns, nf), dtype=bool)          # the lanes that have not met `break` yet
                for l in range(1, nlag):
                    top, bottom = np.zeros((ns, nf)), np.zeros((ns, nf))
                    for w in range(nwin - n, nwin):
                        dm, dm0 = M - mean[w, l], M - mean[w, 0]
                        cv, var = cov[w, l] + dm * dm, cov[w, 0] + dm0 * dm0
                        top = top + cv * cnt[w, l]
                        bottom = bottom + var * cnt[w, l]
                    rho = top / bottom
                    stop = going & (previous < 0) & (rho < 0)
                    length = np.where(stop, length - last_term, length)
                    going = going & ~stop
                    if not going.any():
                        break
                    term = 2.0 * (lags[l] - last_lag) * rho
                    previous = np.where(going, rho, previous)
                    last_term = np.where(going, term, last_term)
                    length = np.where(going, length + term, length)
                    last_lag = np.where(going, float(lags[l]), last_lag)
                e = float(n * width) / length
                out[n - 1] = np.where(length < every, float(n * width) / 3.0 / float(every), e)
        return out

    def windowed(self, width, every, burn, detail=False):
        """(ess[s], nwin[s]); detail=True adds the feature that set the minimum at the winning n"""
        ns, nf = self.nseries, self.nfeat
        ess_out, nwin_out, feat_out = np.zeros(ns), np.zeros(ns, dtype=np.int32), np.full(ns, -1)
        e_of_n = self.feature_ess(width, every, burn)
        if e_of_n is None:
            return (ess_out, nwin_out, feat_out) if detail else (ess_out, nwin_out)
        with np.errstate(all="ignore"):
            for n in range(1, len(e_of_n) + 1):
                e = e_of_n[n - 1]
                worst, worst_f = np.full(ns, 1e100), np.full(ns, -1)
                for f in range(nf):
                    less = e[:, f] < worst
                    worst, worst_f = np.where(less, e[:, f], worst), np.where(less, f, worst_f)
                better = worst > ess_out
                ess_out, nwin_out, feat_out = np.where(better, worst, ess_out), np.where(better, n, nwin_out).astype(np.int32), np.where(better, worst_f, feat_out)
        return (ess_out, nwin_out, feat_out) if detail else (ess_out, nwin_out)

    def report(self, width, every, esslimit, rows=0, initial_rows=0):
        """(ess[s], useful length[s]): every series shares each pass, only `if (e > ess)` is a series' own"""
        min_burn, min_per_window, max_windows = 2, 1000, 20
        steps = self.steps
        width, every = int(width), int(every)
        while width < steps * 0.05:
            width *= 2
        if every < 0:
            every = int(0.5 + (float(steps) - initial_rows) / (rows - initial_rows)) if rows > initial_rows else 1
        if every < 1:
            every = 1
        ess, best_width, nwin = np.zeros(self.nseries), np.zeros(self.nseries, dtype=np.int64), np.zeros(self.nseries, dtype=np.int64)
        if esslimit < 0:
            if width < 0:
                width = every * min_per_window
            while width * (max_windows + min_burn) < steps:
                width *= 2
            ess, nwin = self.windowed(width, every, min_burn)
            best_width[:] = width
        else:
            length, reach = float(steps), esslimit * 3.0
            last_round = False
            while not last_round:
                windows = int(length / (min_per_window * every))
                if windows > max_windows:
                    windows = max_windows
                if windows < 1:
                    break
                width = int(length / windows)
                if width * (windows - 1) > reach * every:
                    windows = int(reach / min_per_window + 1)
                    if windows > max_windows:
                        windows = max_windows
                    if windows > 1:
                        width = int((reach * every) / (windows - 1))
                    else:
                        windows, width = 1, min_per_window * every
                else:
                    last_round = True
                if (length - length / (max_windows + min_burn)) * 0.5 < windows * width:
                    e, n = self.windowed(width, every, int(length / width - windows))
                    better = e > ess
                    ess, nwin, best_width = np.where(better, e, ess), np.where(better, n, nwin), np.where(better, width, best_width)
                every *= 2
        return ess, (best_width * nwin).astype(np.int32)


def series_reader(series):
    """plain series [n, nseries, nfeat]: every step is there"""
    series = np.asarray(series)

    def read(steps):
        return np.ones((len(steps), series.shape[1]), dtype=bool), series[steps]
    return read


def ring_reader(hist, chains, add_every_n):
    """the facade's cold_row on Engine.history() for the history chains `chains` (a slice): nominal step s is saved row
    1 + s // add_every_n, in slot row % capacity if the slot still holds that row"""
    x, row = hist["x"][:, chains], hist["row"][:, chains]
    cap = x.shape[0]

    def read(steps):
        idx = 1 + steps // add_every_n
        slot = idx % cap
        return row[slot] == idx[:, None], x[slot]
    return read


def ring_series(hist, chains, add_every_n, steps):
    """the series [steps, nseries, dim] a complete ring stands for (every nominal step's row must still be there)"""
    valid, x = ring_reader(hist, chains, add_every_n)(np.arange(steps, dtype=np.int64))
    assert valid.all()
    return np.ascontiguousarray(x)


def golden_series(case):
    """the AR(1) series of a tests/golden/ess.json.gz case, regenerated from its recorded helper-stream seed (splitmix64; the
    recipe of tests/test_cxx_facade.py)"""
    dim, n, phi = case["dim"], case["n"], case["phi"]
    k = np.arange(1, 4 * dim * n + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(case["seed"])) + k * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    sym = 2 * ((z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)) - 1
    q4 = sym.reshape(n, dim, 4)
    e = ((q4[..., 0] + q4[..., 1]) + q4[..., 2]) + q4[..., 3]
    x = np.zeros(dim)
    series = np.empty((n, dim))
    ph = np.array(phi)
    for t in range(n):
        x = ph * x + e[t]
        series[t] = x
    return series


def fixture_driver_answers(exe, series, queries):
    """[(ess, length)] of tests/cxx/de_ess_fixture_main.cc `ess` (the facade's host estimator; %.17g round-trips a double)"""
    import subprocess
    n, dim = series.shape
    lines = ["%d %d %d" % (dim, n, len(queries))]
    lines += [" ".join("%.17g" % v for v in row) for row in series]
    lines += ["%d %d %.17g" % (q["width"], q["every"], q["esslimit"]) for q in queries]
    out = subprocess.run([exe, "ess"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert len(rows) == len(queries)
    return [(float(r[0]), int(r[1])) for r in rows]


def build_fixture_driver(d):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(d, "fx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "ptmcmc_amd", "host"),
                           os.path.join(root, "tests", "cxx", "de_ess_fixture_main.cc"), "-L", os.path.join(root, "ptmcmc_amd"), "-lptm_engine",
                           "-Wl,-rpath," + os.path.join(root, "ptmcmc_amd"), "-pthread", "-o", exe])
    return exe
