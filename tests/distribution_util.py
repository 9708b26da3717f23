"""What tests/test_distribution_model_cpu.py and tests/test_gpu_distributions.py share beyond the exact marginals of
tests/distribution_model.py: the CPU checker's twin of every case, the inputs of the differential-evolution cases, and the
measurements the case tables quote.  As a program it repeats those measurements on the checker:

    python tests/distribution_util.py tau        integrated autocorrelation times of cases A (per shape) and C
    python tests/distribution_util.py exchange   exchange acceptance of two rungs a factor 100 apart at 33 and 35 dimensions

(minutes of CPU time, which is why no test repeats them: the tests hold S >= 10 tau against the written numbers)."""
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import distribution_model as M
import oracle_lib as O

THREADS = 8


# ---- cases A on the checker
def make_checker(case, pb, seed, X0, W=None):
    """the checker's twin of a case's engine: X0 [Nt][W][D] exact samples (the checker's chain order is walker-major)"""
    p = O.Problem(pb.D)
    p.set_bounds(*pb.bounds)
    p.set_prior(*pb.prior)
    p.set_gauss(pb.precision, 0.0, pb.mean)
    lad = O.Ladder(p, pb.beta, W=case["W"] if W is None else W, swap_rate=M.SWAP_RATE)
    sig = pb.proposal_sigmas(case["fac"])
    lad.set_proposals([(O.PROP_DIAG, sig[r], case["oned"]) for r in range(pb.Nt)])
    lad.use_philox(seed)
    lad.set_states(X0.transpose(1, 0, 2).reshape(-1, pb.D))
    if case["evolve"] > 0:
        lad.evolve_temps(case["evolve"])
    return lad


_RUNS = {}


def checker_run(case):
    """final snapshots [Nt][runs * W][D] of the case on the checker (cases of one shape and seed share the run), and its counters"""
    key = (id(case["dims"][0]), len(case["dims"]), case["Nt"], case["W"], case["runs"], case["S"], case["seed"], case["fac"], case["oned"], case["evolve"])
    if key not in _RUNS:
        pb = M.problem_of(case)
        snaps, tries, acc, sw_t, sw_a, stuck = [], 0, 0, 0, 0, 0
        for k in range(case["runs"]):
            X0 = pb.exact_samples(case["W"], np.random.default_rng(case["seed"] + k))
            lad = make_checker(case, pb, case["seed"] + k, X0)
            lad.pt_step(case["S"], THREADS)
            snaps.append(lad.x.reshape(case["W"], pb.Nt, pb.D).transpose(1, 0, 2))
            tries += int(lad.ntries.sum()) - lad.N; acc += int(lad.naccept.sum()) - lad.N
            sw_t += int(lad.swap_count.sum()); sw_a += int(lad.swap_accept_count.sum())
            stuck += int((lad.last_type == -1).sum())
        _RUNS[key] = (pb, np.concatenate(snaps, axis=1), tries, acc, sw_t, sw_a, stuck)
    return _RUNS[key]


# ---- cases C: differential evolution with many snooker moves
def de_inputs(case, k):
    """what the k-th run of a C case is configured with, for the engine and the checker alike: the problem, the set's tables [Nt][4], the
    ring capacity, the history rows [10 D][Nt * W][D] (engine chain order) and the start states [Nt][W][D], all exact samples"""
    from ptmcmc_amd.problems import GaussianProblem
    D, Nt, W = case["D"], case["Nt"], case["W"]
    pr = GaussianProblem(D, Nt, M.TMAX)
    rng = np.random.default_rng(case["seed"] + k)
    L = np.linalg.cholesky(pr.cov)
    exact = lambda: (rng.standard_normal((Nt, W, D)) @ L.T) / np.sqrt(np.asarray(pr.beta))[:, None, None]
    g = 2.0 ** np.arange(1, 4)
    cum = np.tile(np.cumsum(np.concatenate([[0.7], 0.3 * g / g.sum()])), (Nt, 1)); cum[:, -1] = 1.0
    scales, odfs = np.tile([-1.0, 0.25, 0.5, 1.0], (Nt, 1)), np.tile([0.0, 0.5, 0.5, 0.5], (Nt, 1))
    init = np.stack([exact().reshape(Nt * W, D) for _ in range(10 * D)])
    cap = 10 * D + 2 * case["S"] // M.DE_EVERY + 8
    return pr, cum, scales, odfs, cap, init, exact()


def de_rungs(case):
    """the rungs a C case compares: the colder half (the reference's own exclusion of the hot ones, test_gpu_statistics.py); of
    evolving ladders, whose interior rungs have another temperature in every ladder, the cold rung alone"""
    return [0] if case["evolve"] > 0 else list(range(case["Nt"] // 2))


def covariance_error(pr, X, rungs):
    """max |C - cov / beta_r| / (sigma_i sigma_j) over the rungs, C the second moments of X [Nt][n][D] about the known mean 0"""
    errs = []
    for r in rungs:
        C = np.einsum("wi,wj->ij", X[r], X[r]) / X.shape[1]
        want = pr.cov / pr.beta[r]
        s = np.sqrt(np.diag(want))
        errs.append(np.abs((C - want) / np.outer(s, s)).max())
    return max(errs)


def make_de_checker(case, k, snooker=M.DE_SNOOKER):
    pr, cum, scales, odfs, cap, init, X0 = de_inputs(case, k)
    D, Nt, W = case["D"], case["Nt"], case["W"]
    p = O.Problem(D)
    p.set_bounds([O.OPEN] * D, [O.OPEN] * D, np.zeros(D), np.zeros(D))
    p.set_prior(pr.types, pr.centers, pr.halfwidths)
    p.set_gauss(pr.P, pr.like0)
    lad = O.Ladder(p, pr.beta, W=W, swap_rate=M.SWAP_RATE, add_every_N=M.DE_EVERY)
    f = np.stack([np.sqrt(np.diag(T @ T.T)) for T in pr.proposal_factors(range(Nt))])
    lad.set_proposals([(O.PROP_DIAG, f[r], 0.0) for r in range(Nt)])
    lad.use_philox(case["seed"] + k)
    lad.enable_history(cap)
    lad.set_states(X0.transpose(1, 0, 2).reshape(-1, D))
    lad.set_mixture(cum, scales, odfs)
    to_oracle = lambda a: a.reshape(Nt, W, D).transpose(1, 0, 2).reshape(-1, D)
    lad.set_de(snooker, 0.3, 4.0, 0.0, init_rows=np.stack([to_oracle(row) for row in init]))
    if case["evolve"] > 0:
        lad.evolve_temps(case["evolve"])
    return pr, lad


def de_checker_run(case, snooker=M.DE_SNOOKER):
    snaps, types = [], set()
    for k in range(case["runs"]):
        pr, lad = make_de_checker(case, k, snooker)
        lad.pt_step(case["S"], THREADS)
        snaps.append(lad.x.reshape(case["W"], case["Nt"], case["D"]).transpose(1, 0, 2))
        types |= set(int(v) for v in np.unique(lad.last_type))
    return pr, np.concatenate(snaps, axis=1), types


# ---- the measurements the case tables quote
def autocorrelation_time(lad, Nt, W, D, steps, maxlag, features=lambda x: x):
    """1 + 2 sum of the autocorrelations up to maxlag of every feature of every rung's chains over `steps` PT steps, averaged over the
    ladders: [Nt][features]"""
    tr = []
    for _ in range(steps):
        lad.pt_step(1, THREADS)
        tr.append(features(lad.x.reshape(W, Nt, D).transpose(1, 0, 2)))
    tr = np.array(tr)
    y = tr - tr.mean(axis=(0, 2), keepdims=True)
    var = tr.var(axis=(0, 2))
    tau = np.ones(var.shape)
    for lag in range(1, maxlag):
        tau += 2 * (y[:-lag] * y[lag:]).mean(axis=(0, 2)) / var
    return tau


def measure_tau():
    np.set_printoptions(precision=0, suppress=True, linewidth=200)
    seen = set()
    for case in M.CASES_A:
        pb = M.problem_of(case)
        if (pb.D, pb.Nt, case["evolve"]) in seen:
            continue
        seen.add((pb.D, pb.Nt, case["evolve"]))
        W = 256 if pb.D > 7 else 512
        lad = make_checker(case, pb, 99, pb.exact_samples(W, np.random.default_rng(5)), W=W)
        tau = autocorrelation_time(lad, pb.Nt, W, pb.D, 1200 if pb.D > 7 else 600, 500 if pb.D > 7 else 150)
        print("A, %d dimensions x %d rungs, evolve %g: tau per rung (slowest dimension) %s" % (pb.D, pb.Nt, case["evolve"], tau.max(axis=1)), flush=True)
    seen = set()
    for case in M.CASES_C:
        if (case["D"], case["Nt"], case["evolve"]) in seen:
            continue
        seen.add((case["D"], case["Nt"], case["evolve"]))
        small = dict(case, W=256, S=400)
        pr, lad = make_de_checker(small, 0)
        feats = lambda x: np.concatenate([x ** 2, x[..., :1] * x[..., 1:2]], axis=-1)     # what the covariance criterion reads
        tau = autocorrelation_time(lad, case["Nt"], 256, case["D"], 400, 150, feats)
        print("C, %d dimensions x %d rungs, evolve %g: tau per rung (slowest square or product) %s" % (case["D"], case["Nt"], case["evolve"], tau.max(axis=1)), flush=True)


def measure_exchange():
    """the two shapes the bin budget (rungs x D x 16 <= 1000) would leave to the 64-dimension kernels: two rungs, Tmax = 100"""
    zoo = M.zoo()
    box = [zoo[0] if d % 2 == 0 else M.Dim(M.UNIFORM, -0.5, 1.5, M.LIMIT, M.LIMIT, -2.0, 1.0, m=-1.8, s=0.6) for d in range(33)]
    for name, dims in (("33 box dimensions (uniform priors, limit bounds, the mass against an edge)", box), ("the zoo five times, 35 dimensions", zoo * 5)):
        case = dict(dims=dims, Nt=2, W=1024, fac=0.6, oned=M.ONE_D_FRAC, evolve=0.0)
        pb = M.Problem(dims, 2, M.TMAX)
        lad = make_checker(case, pb, 7, pb.exact_samples(1024, np.random.default_rng(7)))
        lad.pt_step(1000, THREADS)
        print("%s, 2 rungs x 1024 ladders x 1000 steps: %d of %d exchanges accepted" % (name, lad.swap_accept_count.sum(), lad.swap_count.sum()), flush=True)


if __name__ == "__main__":
    {"tau": measure_tau, "exchange": measure_exchange}[sys.argv[1]]()
