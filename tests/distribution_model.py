"""Exact marginals of the factorising targets the distribution tests sample (tests/test_distribution_model_cpu.py,
tests/test_gpu_distributions.py).  Plain numpy: no engine, no checker.

Target family: a DIAGONAL Gaussian likelihood with a mean, llike(x) = -1/2 sum_d (x_d - m_d)^2 / s_d^2, any prior of
ptm_set_prior per dimension and any boundary.  The posterior of rung r factorises; dimension d has the density

    prior_d(x) * exp(-beta_r (x - m_d)^2 / (2 s_d^2))            on the prior's support

(the acceptance rule of the reference, newlike * beta + newlprior, tempers the likelihood and NOT the prior).  The prior formulas are
those of probability_function.hh / ProbabilityDist.h as include/ptm_engine.h names them (ptm_set_prior: centers c, halfwidths h):

    uniform   1                  on [c - h, c + h]
    gaussian  exp(-(x-c)^2/2h^2) on the whole line
    polar     sin x              on [c - h, c + h] within [0, pi]
    copolar   cos x              on [c - h, c + h] within [-pi/2, pi/2]
    log       1 / x              on [c / h, c * h]

Boundaries do not change a marginal: `limit` invalidates a proposal outside, the reference's two-sided `reflect` folds an overshoot
to the far side of xmin (outside the prior's support: rejected), and `wrap` is a symmetric move on the circle; each is a Metropolis
kernel of the same density.  What they change is how a chain gets there -- a wrong fold or a wrong seam shows in the counts.

Cdfs: closed form where prior and likelihood are Gaussian (precision a / h^2 + b / s^2); otherwise Gauss-Legendre quadrature (16
nodes on each of G panels of the support) in float64.  Every quadrature marginal asserts its own error estimate -- the largest
difference of the cdf from the one on G / 2 panels -- below QUAD_TOL = 1e-9.

Besides the truth, every dimension has NAMED WRONG ALTERNATIVES of the same support (what a specific mistake would converge to):
    prior_ignored    likelihood^beta alone
    prior_twice      prior^2 likelihood^beta   (an independence sampler from the prior WITHOUT its Hastings ratio is invariant for pi * q)
    prior_tempered   (prior likelihood)^beta
for the dimensions whose prior is not uniform, and
    untruncated      the Gaussian likelihood^beta on the whole line
for a uniform dimension with `limit` or `reflect` boundaries."""
import math

import numpy as np

OPEN, LIMIT, REFLECT, WRAP = 0, 1, 2, 3                      # boundary types of include/ptm_engine.h
UNIFORM, GAUSSIAN, POLAR, COPOLAR, LOG = 1, 2, 3, 4, 5       # prior types

K_BINS = 16          # equiprobable bins per (rung, dimension)
Z_BOUND = 5.0        # acceptance: max |z| over all rungs, dimensions and bins
Z_REJECT = 15.0      # discrimination: every alternative is rejected by this much on at least one rung
QUAD_TOL = 1e-9

_GL_X, _GL_W = np.polynomial.legendre.leggauss(16)
_erfc = np.vectorize(math.erfc, otypes=[float])


def geometric_ladder(n_rungs, tmax):
    """chain.cc:1181-1183,1340, the very operations of ptmcmc_amd.engine.geometric_ladder (no engine import here)"""
    tratio = math.exp(math.log(tmax) / (n_rungs - 1)) if n_rungs > 1 else 1.0
    t, beta = 1.0, [1.0]
    for _ in range(1, n_rungs):
        t = t * tratio
        beta.append(1 / t)
    return np.array(beta)


class Dim:
    """one dimension of a problem: its prior (type, center, halfwidth), its boundary (types, xmin, xmax) and its likelihood factor
    (mean m, width s)"""

    def __init__(self, prior, c, h, lo=OPEN, hi=OPEN, xmin=0.0, xmax=0.0, m=0.0, s=1.0):
        self.prior, self.c, self.h, self.lo, self.hi, self.xmin, self.xmax, self.m, self.s = prior, c, h, lo, hi, xmin, xmax, m, s

    @property
    def support(self):
        c, h = self.c, self.h
        if self.prior == UNIFORM:
            return c - h, c + h
        if self.prior == POLAR:
            return max(c - h, 0.0), min(c + h, math.pi)
        if self.prior == COPOLAR:
            return max(c - h, -math.pi / 2), min(c + h, math.pi / 2)
        if self.prior == LOG:
            return c / h, c * h
        return -math.inf, math.inf

    def log_prior(self, x):
        """unnormalised, on the support"""
        if self.prior == UNIFORM:
            return np.zeros_like(x)
        if self.prior == GAUSSIAN:
            return -0.5 * ((x - self.c) / self.h) ** 2
        if self.prior == POLAR:
            return np.log(np.sin(x))
        if self.prior == COPOLAR:
            return np.log(np.cos(x))
        if self.prior == LOG:
            return -np.log(x)
        raise ValueError(self.prior)

    def log_like(self, x):
        return -0.5 * ((x - self.m) / self.s) ** 2


class GaussianMarginal:
    """closed form: N(mu, sigma^2) on the whole line"""

    def __init__(self, mu, sigma):
        self.mu, self.sigma, self.lo, self.hi = mu, sigma, -math.inf, math.inf

    def cdf(self, x):
        z = (np.asarray(x, dtype=np.float64) - self.mu) / (self.sigma * math.sqrt(2.0))
        z = np.clip(z, -30.0, 30.0)                               # (erfc of an infinite edge: 0 or 2)
        return 0.5 * _erfc(-z)

    def ppf(self, u):
        """bisection on the closed form (a few values only: bin edges)"""
        u = np.atleast_1d(np.asarray(u, dtype=np.float64))
        a, b = np.full(u.shape, self.mu - 12 * self.sigma), np.full(u.shape, self.mu + 12 * self.sigma)
        for _ in range(80):
            mid = 0.5 * (a + b)
            below = self.cdf(mid) < u
            a, b = np.where(below, mid, a), np.where(below, b, mid)
        return 0.5 * (a + b)


class QuadMarginal:
    """density exp(logf) on [lo, hi] by quadrature: cdf, inverse cdf, and the error estimate of the cdf"""

    def __init__(self, logf, lo, hi, panels=512):
        self.logf, self.lo, self.hi, self.G = logf, float(lo), float(hi), panels
        assert math.isfinite(self.lo) and math.isfinite(self.hi) and self.hi > self.lo
        probe = np.linspace(self.lo, self.hi, 4097)[1:-1]
        self.shift = float(np.max(logf(probe)))                   # keeps exp in range; cancels in every ratio
        self.e, self.C = self._tabulate(panels)
        self.Z = self.C[-1]
        # the error estimate: the same cdf from half as many panels, at the fine grid's panel edges and midpoints
        e2, C2 = self._tabulate(panels // 2)
        at = np.concatenate([self.e, 0.5 * (self.e[1:] + self.e[:-1])])
        self.quad_error = float(np.abs(self._cdf_on(at, self.e, self.C) - self._cdf_on(at, e2, C2)).max())
        assert self.quad_error < QUAD_TOL, "quadrature cdf not converged: %g" % self.quad_error

    def _f(self, x):
        return np.exp(self.logf(x) - self.shift)

    def _integral(self, a, b):
        """Gauss-Legendre on [a, b], elementwise"""
        half, mid = 0.5 * (b - a), 0.5 * (b + a)
        return half * (self._f(mid[..., None] + half[..., None] * _GL_X) * _GL_W).sum(axis=-1)

    def _tabulate(self, G):
        e = np.linspace(self.lo, self.hi, G + 1)
        return e, np.concatenate([[0.0], np.cumsum(self._integral(e[:-1], e[1:]))])

    def _cdf_on(self, x, e, C):
        x = np.clip(np.asarray(x, dtype=np.float64), self.lo, self.hi)
        j = np.clip(np.searchsorted(e, x, side="right") - 1, 0, len(e) - 2)
        return (C[j] + self._integral(e[j], x)) / C[-1]

    def cdf(self, x):
        return self._cdf_on(x, self.e, self.C)

    def ppf(self, u):
        """safeguarded Newton inside the panel that holds the quantile; the residual is asserted"""
        u = np.atleast_1d(np.asarray(u, dtype=np.float64))
        t = u * self.Z
        j = np.clip(np.searchsorted(self.C, t, side="right") - 1, 0, self.G - 1)
        a, b = self.e[j], self.e[j + 1]
        x = a + (b - a) * (t - self.C[j]) / np.maximum(self.C[j + 1] - self.C[j], 1e-300)
        for _ in range(12):
            r = self.C[j] + self._integral(a, x) - t
            x = np.clip(x - r / np.maximum(self._f(x), 1e-300), a, b)
        assert np.abs(self.cdf(x) - u).max() < 1e-11
        return x


def _gauss_params(dim, a, b):
    """prior^a likelihood^b of a Gaussian-prior dimension: precision a / h^2 + b / s^2"""
    tau = a / dim.h ** 2 + b / dim.s ** 2
    return (a * dim.c / dim.h ** 2 + b * dim.m / dim.s ** 2) / tau, 1.0 / math.sqrt(tau)


def marginal(dim, a, b, quadrature=False):
    """the density prior^a likelihood^b of one dimension on the prior's support (a = 1, b = beta: the truth)"""
    lo, hi = dim.support
    if dim.prior == GAUSSIAN:
        mu, sigma = _gauss_params(dim, a, b)
        if not quadrature:
            return GaussianMarginal(mu, sigma)
        lo, hi = mu - 12 * sigma, mu + 12 * sigma                 # (2e-33 of the mass lies outside)
    return QuadMarginal(lambda x: a * dim.log_prior(x) + b * dim.log_like(x), lo, hi)


def alternatives(dim, beta):
    """name -> marginal of the wrong alternatives that apply to this dimension"""
    if dim.prior != UNIFORM:
        return {"prior_ignored": marginal(dim, 0.0, beta), "prior_twice": marginal(dim, 2.0, beta), "prior_tempered": marginal(dim, beta, beta)}
    if dim.lo in (LIMIT, REFLECT):
        return {"untruncated": GaussianMarginal(dim.m, dim.s / math.sqrt(beta))}
    return {}


def zoo():
    """Seven dimensions (padded to 8 by the engine).  The limit interval contains 0 (state::add is invalid on a space whose origin
    violates a `limit` bound); the polar and log supports, which exclude 0, take reflect / open boundaries; the prior's ratio across
    every bounded support is above e^-6.3 (log sin 0.002 = -6.21; the min_prior cut is e^-30); every likelihood width is comparable to its prior's width."""
    pi = math.pi
    return [
        Dim(UNIFORM, 0.5, 1.5, LIMIT, LIMIT, -1.0, 2.0, m=1.8, s=0.6),                       # mass piled against the upper edge
        Dim(UNIFORM, -0.5, 1.5, REFLECT, REFLECT, -2.0, 1.0, m=-1.8, s=0.6),                 # ... against the lower edge
        Dim(UNIFORM, 0.0, 1.0, WRAP, WRAP, -1.0, 1.0, m=0.9, s=0.5),                         # mass on both sides of the seam at +-1
        Dim(GAUSSIAN, 0.5, 1.0, m=-0.5, s=1.0),
        Dim(POLAR, pi / 2, pi / 2 - 0.002, REFLECT, REFLECT, 0.002, pi - 0.002, m=pi / 2 - 1.2, s=0.6),
        Dim(COPOLAR, 0.0, pi / 2 - 0.002, REFLECT, REFLECT, -pi / 2 + 0.002, pi / 2 - 0.002, m=-1.2, s=0.6),
        Dim(LOG, 3.0, 6.0, m=4.0, s=4.0),
    ]


class Problem:
    """dimensions x a geometric ladder: everything both samplers are configured from, and the exact marginals of every
    (rung, dimension).  Dimensions that repeat share their marginals."""

    def __init__(self, dims, n_rungs, tmax=100.0):
        self.dims, self.D, self.Nt = list(dims), len(dims), n_rungs
        self.beta = geometric_ladder(n_rungs, tmax)
        cache = {}
        self.truth, self.alts, self.edges = {}, {}, {}
        for r in range(n_rungs):
            for d, dim in enumerate(self.dims):
                key = (r, id(dim)) if self.dims.count(dim) > 1 else (r, d)
                if key not in cache:
                    t = marginal(dim, 1.0, self.beta[r])
                    inner = t.ppf(np.arange(1, K_BINS) / K_BINS)
                    cache[key] = (t, alternatives(dim, self.beta[r]), np.concatenate([[t.lo], inner, [t.hi]]))
                self.truth[r, d], self.alts[r, d], self.edges[r, d] = cache[key]

    # -- what the samplers are configured with
    @property
    def bounds(self):
        return ([v.lo for v in self.dims], [v.hi for v in self.dims], np.array([v.xmin for v in self.dims]), np.array([v.xmax for v in self.dims]))

    @property
    def prior(self):
        return ([v.prior for v in self.dims], np.array([v.c for v in self.dims]), np.array([v.h for v in self.dims]))

    @property
    def precision(self):
        return np.diag([1.0 / v.s ** 2 for v in self.dims])

    @property
    def mean(self):
        return np.array([v.m for v in self.dims])

    def proposal_sigmas(self, fac=0.6):
        """diagonal Gaussian proposals [Nt][D]: fac s_d / sqrt(max(beta, 0.1))"""
        s = np.array([v.s for v in self.dims])
        return fac * s[None, :] / np.sqrt(np.maximum(self.beta, 0.1))[:, None]

    def log_like(self, X):
        """the same diagonal Gaussian for a likelihood handed over as a function: X [n][D] -> [n]"""
        return -0.5 * (((np.asarray(X) - self.mean) / np.array([v.s for v in self.dims])) ** 2).sum(axis=-1)

    # -- the harness
    def exact_samples(self, n, rng):
        """[Nt][n][D]: inverse-cdf samples of every (rung, dimension)"""
        X = np.empty((self.Nt, n, self.D))
        for r in range(self.Nt):
            for d, dim in enumerate(self.dims):
                sampler = self.truth[r, d] if dim.prior != GAUSSIAN else marginal(dim, 1.0, self.beta[r], quadrature=True)
                X[r, :, d] = sampler.ppf(rng.uniform(size=n))
        return X

    def counts(self, X):
        """X [Nt][n][D] -> counts [Nt][D][K]; a sample outside the support is an error"""
        X = np.asarray(X)
        out = np.zeros((self.Nt, self.D, K_BINS), dtype=np.int64)
        for (r, d), e in self.edges.items():
            x = X[r, :, d]
            assert (x >= e[0]).all() and (x <= e[-1]).all(), "rung %d, dimension %d: a sample outside the support" % (r, d)
            out[r, d] = np.bincount(np.clip(np.searchsorted(e, x, side="right") - 1, 0, K_BINS - 1), minlength=K_BINS)
        return out

    def alt_probs(self, r, d, name):
        """the alternative's probability of each of the truth's bins"""
        return np.maximum(np.diff(self.alts[r, d][name].cdf(self.edges[r, d])), 1e-300)

    def applicable(self, exclude=()):
        """(dimension, name) of every alternative (but those excluded by name)"""
        return [(d, name) for d in range(self.D) for name in sorted(self.alts[0, d]) if name not in exclude]


def z_scores(counts, n):
    """(count - n / K) / sqrt(n (1 / K) (1 - 1 / K)): exactly binomial for n independent samples"""
    p = 1.0 / K_BINS
    return (np.asarray(counts) - n * p) / math.sqrt(n * p * (1 - p))


def alt_z(counts, n, p_alt):
    return (np.asarray(counts) - n * p_alt) / np.sqrt(n * p_alt * (1 - p_alt))


def design_shift(n, p_alt):
    """the expected shift of the worst bin if the truth holds and the alternative is tested: n |p_alt - 1/K| / sqrt(n p_alt (1 - p_alt))"""
    return float((n * np.abs(p_alt - 1.0 / K_BINS) / np.sqrt(n * p_alt * (1 - p_alt))).max())


def worst_z(pb, counts, n, rungs=None):
    """(max |z|, (rung, dimension, bin)) over the given rungs"""
    z = np.abs(z_scores(counts, n))
    rungs = list(range(pb.Nt)) if rungs is None else list(rungs)
    sub = z[rungs]
    k = np.unravel_index(np.argmax(sub), sub.shape)
    return float(sub[k]), (rungs[k[0]], int(k[1]), int(k[2]))


def rejections(pb, counts, n, rungs=None, exclude=()):
    """{(dimension, name): the largest |z| of the counts against the alternative over the rungs}"""
    rungs = range(pb.Nt) if rungs is None else rungs
    return {(d, name): max(float(np.abs(alt_z(counts[r, d], n, pb.alt_probs(r, d, name))).max()) for r in rungs) for d, name in pb.applicable(exclude)}


def design_shifts(pb, n, rungs=None, exclude=()):
    """{(dimension, name): the largest design shift over the rungs} -- from the exact cdfs alone"""
    rungs = range(pb.Nt) if rungs is None else rungs
    return {(d, name): max(design_shift(n, pb.alt_probs(r, d, name)) for r in rungs) for d, name in pb.applicable(exclude)}


def judged(case):
    """(rungs, alternatives left out) a case is judged by.  An evolving ladder's interior rungs have another temperature in every ladder:
    its cold rung (beta = 1 always) is the test, and there prior_tempered IS the truth, so it is no alternative of such a case."""
    return ([0], ("prior_tempered",)) if case["evolve"] > 0 else (list(range(case["Nt"])), ())


# ---- the cases of tests/test_gpu_distributions.py, as plain data (tests/test_distribution_model_cpu.py holds every one of them to
# the design condition and runs those the CPU checker can run).
#   dims     the problem's dimensions          Nt, W    rungs, ladders per engine        runs    engines whose final snapshots are pooled
#   S        PT steps before the one snapshot  tau      the integrated autocorrelation time, in PT steps, of the slowest (rung, dimension),
#                                                       measured once on the CPU checker at this shape (S >= 10 tau);
#                                                       tests/distribution_util.py repeats the measurements as a program
#   kernel   what must be in the engine's step or sweep kernel name             opts   Engine keyword arguments
# Every case: geometric ladder to Tmax = 100, swap_rate 0.2, diagonal Gaussian proposals 0.6 s_d / sqrt(max(beta, 0.1)), half of
# the moves one-dimensional.
ONE_D_FRAC = 0.5
EVOLVE_RATE = 0.01
SWAP_RATE = 0.2
TMAX = 100.0


def _case(name, dims, Nt, W, S, tau, kernel, runs=1, seed=0, member=None, like="gauss", fac=0.6, oned=ONE_D_FRAC, evolve=0.0, **opts):
    return dict(name=name, dims=dims, Nt=Nt, W=W, S=S, tau=tau, kernel=kernel, runs=runs, seed=0xD157 + 1000 * seed, member=member, like=like,
                fac=fac, oned=oned, evolve=evolve, opts=opts)


_ZOO = zoo()
_TWO_LAUNCH = dict(time_kernels=True)   # keeps step() on exchange kernel + sweep kernel where a step kernel would take the shape

# Cases A: priors and bounds under Gaussian proposals, one per kernel family that carries them.  tau: measured on the checker (512
# ladders x 600..1200 steps, autocorrelations summed to lag 150 at 7 dimensions, 500 at 14 and 21): 56 / 216 / 482 PT steps on the
# cold rung at 7 / 14 / 21 dimensions (a dimension is moved by about every 1 / D-th accepted proposal).
# (`python tests/distribution_util.py tau` repeats the measurement.)
# Not here, and why: sweep_lanes_kernel<64, ...> (35 dimensions) and sweep_mfma64_kernel<..., true, ...> (33 or more, box problems).  The bin
# budget rungs x D x 16 <= 1000 leaves them two rungs (and 1056 / 1120 bins even so), and two rungs a factor 100 apart in temperature do
# not exchange at such dimensions -- measured on the checker, 2 rungs x 1024 ladders x 1000 steps (`distribution_util.py exchange`): 0 of
# 204591 exchanges accepted with 33 box dimensions, 2 of 204591 with the zoo five times -- so the movement condition cannot hold within
# the budget.  The 21-dimension case takes 3 rungs: 1008 bins, a false-alarm chance of 5.8e-4.
CASES_A = [
    _case("sweep_kernel, whole waves per rung", _ZOO, 4, 4096, 600, 56, "sweep_kernel<8, 1, true, false>", seed=1, **_TWO_LAUNCH),
    _case("sweep_kernel, ragged population", _ZOO, 4, 4097, 600, 56, "sweep_kernel<8, 1, false, false>", seed=2, **_TWO_LAUNCH),
    _case("lanes kernel, 16 padded dimensions", _ZOO * 2, 4, 4097, 2200, 216, "sweep_lanes_kernel<16, 1, true>", seed=3, **_TWO_LAUNCH),
    _case("fused small-ladder kernel", _ZOO, 4, 4096, 600, 56, "ladder_steps_kernel<8, 1", seed=1),
    _case("persistent ladder kernel, any boundary and prior", _ZOO, 4, 256, 600, 56, "ladder_persistent_kernel<8, 1, 19>", runs=16, seed=5),
    _case("32-dimension matrix-core kernel, general build", _ZOO * 3, 3, 4096, 5000, 482, "sweep_mfma32_kernel<2, false, 2", seed=6),
    # evolving ladders (the sampler's rate 0.01): the cold rung alone is judged, so n = 64 x 256 = 16384, at which every alternative that
    # applies there shifts a bin by 15 or more (untruncated 15.2; 7.6 at 4096 would not do)
    _case("persistent ladder kernel, evolving ladders", _ZOO, 4, 256, 600, 56, "ladder_persistent_kernel<8, 1, 23>", runs=64, seed=7, evolve=EVOLVE_RATE),
]

# Cases B: the prior-draw member.  The checker knows no such member, so tau is not measured but bounded: the member alone is an
# independence sampler, whose autocorrelation time is at most 2 / a with a its acceptance rate -- 0.022 on the cold rung (the mean of
# min(1, likelihood ratio) over exact samples and prior draws), 0.41 / 0.84 / 0.96 above it -- and 4 of 5 steps move: 2 / 0.022 / 0.8 = 114.
# The slowest relaxation of that case is slower, though: a cold chain near the likelihood's peak accepts a draw in 200 or so and is seldom
# exchanged away.  A plain numpy emulation of the case (the candidate selection of chain.cc:1410-1420, independence moves from exact prior
# draws) leaves 142 / 18 / 3 / 0 of 4096 cold chains without an accepted draw after 500 / 1000 / 1500 / 2000 steps: a factor e every 260
# steps.  tau = 260 is that time, and S = 4000 puts the expected number of chains whose last_type is still -1 at 1e-4 (the movement condition).
# In a set {Gaussian 0.7, prior 0.3} the Gaussian member alone, at its share, gives the checker's tau / 0.7 (prior draws only shorten it).
CASES_B = [
    _case("prior member alone, sweep_kernel", _ZOO, 4, 4096, 4000, 260, "sweep_kernel<8, 1, true, false>", seed=11, member="alone"),
    _case("{Gaussian 0.7, prior 0.3}, sweep_kernel", _ZOO, 4, 4096, 800, 80, "sweep_kernel<8, 1, true, false>", seed=12, member=(0.3, 0.0)),
    _case("{Gaussian 0.7, prior 0.3}, lanes kernel", _ZOO * 2, 4, 4097, 3100, 309, "sweep_lanes_kernel<16, 1, true>", seed=13, member=(0.3, 0.0)),
    _case("thermal shares, sweep_kernel", _ZOO, 4, 4096, 800, 80, "sweep_kernel<8, 1, true, false>", seed=14, member=(0.3, 0.5)),
    _case("thermal shares, lanes kernel", _ZOO * 2, 4, 4097, 3100, 309, "sweep_lanes_kernel<16, 1, true>", seed=15, member=(0.3, 0.5)),
    _case("{Gaussian 0.7, prior 0.3} around a host-callback likelihood", _ZOO, 4, 4096, 800, 80, "sweep_kernel<8, 1, true, false>", seed=16,
          member=(0.3, 0.0), like="host"),
    # (a torch function: a child process that imports torch before the engine library)
    _case("{Gaussian 0.7, prior 0.3} around a device likelihood", _ZOO, 4, 4096, 800, 80, "sweep_kernel<8, 1, true, false> + device likelihood", seed=17,
          member=(0.3, 0.0), like="device"),
]

# Cases C: differential evolution with many snooker moves (Hastings term (r'/r)^(D-1)) on ptmcmc_amd.problems.GaussianProblem
# (correlated, the untruncated box), in every family that draws it.  Set {differential evolution 0.7, three Gaussians 0.3}, history of
# 10 D rows of exact samples per chain, a row saved every DE_EVERY steps.  Criterion: the covariance of the one final snapshot, colder
# half of the rungs (the hot ones are the reference's own exclusion: test_gpu_statistics.py), against cov / beta_r at 5 sigma of the
# estimator at the exact n: 5 sqrt(2 / n); of evolving ladders the cold rung alone.  tau: the checker's, of the squares and products x_i x_j
# the criterion reads, slowest rung (the hottest): 34 at 6 dimensions x 10 rungs (30 evolving), 85 at 14 x 8 (`distribution_util.py tau`).
DE_SNOOKER = 0.5
DE_EVERY = 10


def _case_c(name, D, Nt, W, S, tau, kernel, runs=1, seed=0, evolve=0.0, **opts):
    return dict(name=name, D=D, Nt=Nt, W=W, S=S, tau=tau, kernel=kernel, runs=runs, seed=0xDE00 + 1000 * seed, evolve=evolve, opts=opts)


CASES_C = [
    _case_c("sweep_kernel", 6, 10, 4096, 350, 34, "sweep_kernel<8, 1, true, false>", seed=1, **_TWO_LAUNCH),
    # (whole waves with differential evolution take the lanes kernel from 16 padded dimensions on, up to 2^19 lanes: 8 rungs x 4096 x 16)
    _case_c("lanes kernel, whole waves", 14, 8, 4096, 900, 85, "sweep_lanes_kernel<16, 1, true>", seed=2, **_TWO_LAUNCH),
    _case_c("fused small-ladder kernel", 6, 10, 4096, 350, 34, "ladder_steps_kernel<8, 1", seed=1),
    _case_c("persistent ladder kernel", 6, 10, 256, 350, 34, "ladder_persistent_kernel<8, 1, 11>", runs=16, seed=4),
    # (evolving ladders: the cold rung's covariance alone)
    _case_c("persistent ladder kernel, evolving ladders", 6, 10, 256, 350, 34, "ladder_persistent_kernel<8, 1, 15>", runs=16, seed=5, evolve=EVOLVE_RATE),
]

ALL_CASES = CASES_A + CASES_B
CHECKER_CASES = CASES_A               # (everything the checker can run: all but the prior-draw member)

_PROBLEMS = {}


def problem_of(case):
    key = (id(case["dims"][0]), len(case["dims"]), case["Nt"])
    if key not in _PROBLEMS:
        _PROBLEMS[key] = Problem(case["dims"], case["Nt"], TMAX)
    return _PROBLEMS[key]
