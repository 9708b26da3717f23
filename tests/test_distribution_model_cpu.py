"""The harness and the case design of tests/test_gpu_distributions.py, without a GPU.

  harness    exact samples alone pass their own bin test; the quadrature cdf of the Gaussian-prior dimension agrees with the closed
             form; every quadrature marginal's error estimate (halving the grid) is below 1e-9
  design     a condition, not a measurement: from the exact cdfs alone, at each GPU case's own n, the expected shift of the worst bin
             under every alternative of every dimension that has one is at least 15 on at least one rung (three times the acceptance
             bound) -- a case that could not tell the alternatives apart does not ship
  checker    every case the CPU checker can run (all but the prior-draw member) goes through the same harness with oracle_lib.Ladder
             at the GPU case's seed, shape and start states and must stay within the bound.  The checker is pinned to the real reference
             (test_oracle_golden.py): this validates the harness, and shows that the reference alone passes."""
import numpy as np
import pytest

import distribution_model as M
from distribution_util import checker_run, covariance_error, de_checker_run, de_rungs


_DE_SHAPES = {}          # (cases of one shape and seed are one run of the checker)
for _c in M.CASES_C:
    _DE_SHAPES.setdefault((_c["D"], _c["Nt"], _c["W"], _c["runs"], _c["S"], _c["seed"], _c["evolve"]), []).append(_c)


@pytest.mark.parametrize("case", [v[0] for v in _DE_SHAPES.values()], ids=[" = ".join(c["name"] for c in v) for v in _DE_SHAPES.values()])
def test_the_checker_keeps_the_covariance_under_differential_evolution(case):
    """... which decides that a snooker share of 0.5 is a fair null: the checker itself stays inside the bound with it (the colder half
    of the rungs; of evolving ladders the cold rung)"""
    pr, X, types = de_checker_run(case)
    n = X.shape[1]
    assert n >= 4096 and case["S"] >= 10 * case["tau"]
    bound = 5.0 * np.sqrt(2.0 / n)
    err = covariance_error(pr, X, de_rungs(case))
    print("%s on the checker, snooker %.1f: max |C - cov / beta| / (sigma_i sigma_j) = %.4f over rungs %s (bound %.4f, n = %d), type codes %s"
          % (case["name"], M.DE_SNOOKER, err, de_rungs(case), bound, n, sorted(types)))
    assert err < bound
    assert types & {0, 10}, types          # differential-evolution moves were accepted


# ---- harness
@pytest.fixture(scope="module")
def zoo4():
    return M.Problem(M.zoo(), 4)


def test_exact_samples_pass_their_own_bin_test(zoo4):
    n = 4096
    X = zoo4.exact_samples(n, np.random.default_rng(2024))
    c = zoo4.counts(X)
    assert c.sum(axis=-1).min() == n == c.sum(axis=-1).max()
    z, where = M.worst_z(zoo4, c, n)
    print("exact samples: worst |z| = %.2f at (rung, dimension, bin) %s over %d bins" % (z, where, c.size))
    assert z <= M.Z_BOUND
    # ... and the same counts reject every alternative (prior_tempered IS the truth on the cold rung: beta = 1)
    rej = M.rejections(zoo4, c, n)
    assert min(rej.values()) >= M.Z_REJECT, rej
    cold = M.rejections(zoo4, c, n, rungs=[0])
    assert max(v for (d, name), v in cold.items() if name == "prior_tempered") <= M.Z_BOUND


def test_quadrature_agrees_with_the_closed_form_and_states_its_error(zoo4):
    dim = zoo4.dims[3]
    assert dim.prior == M.GAUSSIAN
    for beta in zoo4.beta:
        for a, b in ((1.0, beta), (0.0, beta), (2.0, beta), (beta, beta)):
            q, g = M.marginal(dim, a, b, quadrature=True), M.marginal(dim, a, b)
            x = np.linspace(g.mu - 8 * g.sigma, g.mu + 8 * g.sigma, 2001)
            assert np.abs(q.cdf(x) - g.cdf(x)).max() < M.QUAD_TOL
            u = np.array([1e-6, 0.01, 0.3, 0.5, 0.9, 1 - 1e-6])
            assert np.abs(g.cdf(q.ppf(u)) - u).max() < M.QUAD_TOL and np.abs(g.cdf(g.ppf(u)) - u).max() < 1e-12
    errs = [t.quad_error for t in zoo4.truth.values() if isinstance(t, M.QuadMarginal)]
    errs += [t.quad_error for alts in zoo4.alts.values() for t in alts.values() if isinstance(t, M.QuadMarginal)]
    assert len(errs) >= 4 * (6 + 9) and max(errs) < M.QUAD_TOL
    print("largest quadrature error estimate of %d marginals: %.2e" % (len(errs), max(errs)))


def test_the_uniform_truncated_marginal_against_its_closed_form(zoo4):
    """a uniform prior with a Gaussian likelihood: (Phi(x) - Phi(lo)) / (Phi(hi) - Phi(lo))"""
    for r, beta in enumerate(zoo4.beta):
        for d in (0, 1, 2):
            dim, t = zoo4.dims[d], zoo4.truth[r, d]
            g = M.GaussianMarginal(dim.m, dim.s / np.sqrt(beta))
            x = np.linspace(t.lo, t.hi, 1001)
            want = (g.cdf(x) - g.cdf(t.lo)) / (g.cdf(t.hi) - g.cdf(t.lo))
            assert np.abs(t.cdf(x) - want).max() < M.QUAD_TOL


def test_the_zoo_respects_the_two_traps(zoo4):
    """every `limit` interval contains the origin; the prior's ratio across every bounded support is far above the min_prior cut"""
    for dim in zoo4.dims:
        if M.LIMIT in (dim.lo, dim.hi):
            assert dim.xmin < 0 < dim.xmax
        lo, hi = dim.support
        if np.isfinite(lo):
            lp = dim.log_prior(np.linspace(lo, hi, 1001))
            assert lp.max() - lp.min() < 10.0 < 30.0


# ---- design
@pytest.mark.parametrize("case", M.ALL_CASES, ids=[c["name"] for c in M.ALL_CASES])
def test_design_condition(case):
    pb = M.problem_of(case)
    n = case["W"] * case["runs"]
    assert n >= 4096 and case["S"] >= 10 * case["tau"]
    # the issue's budget is 1000 bins for a false-alarm chance <= 6e-4; the 21-dimension case has 3 rungs x 21 x 16 = 1008, and
    # 1008 bins x 5.7e-7 (two-sided 5 sigma) = 5.8e-4 still meets it
    rungs, exclude = M.judged(case)
    assert len(rungs) * pb.D * M.K_BINS <= 1008
    shifts = M.design_shifts(pb, n, rungs, exclude)
    assert shifts and len(shifts) == len(pb.applicable(exclude))
    assert all(d in {k[0] for k in shifts} for d in range(pb.D) if pb.dims[d].prior != M.UNIFORM)
    worst = min(shifts, key=shifts.get)
    print("%s: n = %d, smallest design shift %.1f (%s)" % (case["name"], n, shifts[worst], worst))
    assert shifts[worst] >= M.Z_REJECT, shifts


# ---- checker
@pytest.mark.parametrize("case", M.CHECKER_CASES, ids=[c["name"] for c in M.CHECKER_CASES])
def test_the_checker_keeps_every_marginal(case):
    pb, X, tries, acc, sw_t, sw_a, stuck = checker_run(case)
    n = X.shape[1]
    assert n == case["W"] * case["runs"]
    rungs, exclude = M.judged(case)
    c = pb.counts(X)
    z, where = M.worst_z(pb, c, n, rungs)
    rej = M.rejections(pb, c, n, rungs, exclude)
    print("%s on the checker: worst |z| = %.2f at %s, n = %d, acceptance %.3f, exchanges %.3f, weakest rejection %.1f"
          % (case["name"], z, where, n, acc / tries, sw_a / max(1, sw_t), min(rej.values())))
    assert z <= M.Z_BOUND
    assert min(rej.values()) >= M.Z_REJECT, rej
    assert 0.05 * tries < acc < 0.95 * tries and sw_a > 0 and stuck == 0
