"""Timings around the prior member of the proposal set (ptm_set_proposal_prior_draw), bare engine, us per PT step (best of 3 batches).
  population D Nt W steps   the default recipe (80 % differential evolution + six Gaussians, evolving ladder, history, MAP: tools/de_probe.py's
                            population with 10 D initial rows) WITHOUT a prior member -- what the branch in the sweep kernels costs the
                            workloads that do not use it; runs on any build of the engine (--tree DIR: the checkout whose ptmcmc_amd package is imported)
  polar D Nt W steps share  a set {prior member `share`, Gaussian}: all-uniform prior against the same with a polar and a copolar
                            dimension (64 bisections each per draw) -- the difference is what those two draws cost a step
usage: python tools/prior_draw_probe.py [--tree DIR] population|polar [D] [Nt] [W] [steps] [share]"""
import os
import sys
import time
TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 2 and sys.argv[1] == "--tree":
    TREE = os.path.abspath(sys.argv[2])
    del sys.argv[1:3]
sys.path.insert(0, TREE)
import numpy as np
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem


def timed(e, n, warm=100, reps=3):
    e.step(warm); e.sync()
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        e.step(n); e.sync()
        best = min(best, (time.perf_counter() - t0) / n)
    return best * 1e6


def population(D, Nt, W, n):
    warm, reps, every = 100, 3, 2
    cap = (warm + reps * n) * 2 // every + 64
    pr = GaussianProblem(D, Nt, 1e6)
    e = E.Engine(D, Nt, W, add_every_n=every, history_rungs=Nt, history_capacity=cap, map_rungs=Nt)
    pr.configure(e, E.PROP_DIAG)
    K = 6
    g = 2.0 ** np.arange(1, K + 1)
    shares = np.concatenate([[0.8], 0.2 * g / g.sum()])
    cum = np.tile(np.cumsum(shares), (Nt, 1)); cum[:, -1] = 1.0
    scales = np.tile(np.concatenate([[-1.0], 4.0 ** -np.arange(K)[::-1]]), (Nt, 1))
    odfs = np.tile(np.concatenate([[0.0], np.full(K, 0.5)]), (Nt, 1))
    e.set_proposal_mixture(cum, scales, odfs)
    e.init_from_prior()
    rng = np.random.default_rng(1)
    init = rng.uniform(-1.0, 1.0, size=(10 * D, Nt * W, D)) * np.asarray(pr.halfwidths)[None, None, :] * 0.02
    e.set_proposal_de(0.1, 0.3, 4.0, 0.0, init_rows=init)
    del init
    e.set_evolve_temps(0.01)
    us = timed(e, n, warm, reps)
    t, a = e.counter_sums()
    print("population D=%d %dx%d default recipe: %.2f us per PT step   [%s]  MH acceptance %.3f" % (D, Nt, W, us, e.step_kernel_name, a / max(1, t)), flush=True)
    e.close()


def polar(D, Nt, W, n, share):
    out = []
    for trig in (False, True):
        pr = GaussianProblem(D, Nt, 1e3)
        e = E.Engine(D, Nt, W)
        pr.configure(e, E.PROP_DIAG)
        types, cen, hw = [E.PRIOR_UNIFORM] * D, [0.0] * D, [3.0 * float(np.sqrt(pr.cov[d, d])) for d in range(D)]
        if trig:   # a polar dimension on (0.2, pi - 0.2) and a copolar one on (-1.1, 1.3)
            types[D - 2], cen[D - 2], hw[D - 2] = E.PRIOR_POLAR, np.pi / 2, np.pi / 2 - 0.2
            types[D - 1], cen[D - 1], hw[D - 1] = E.PRIOR_COPOLAR, 0.1, 1.2
        e.set_prior(types, cen, hw)
        e.set_proposal_mixture(np.tile([share, 1.0], (Nt, 1)), np.ones((Nt, 2)), np.zeros((Nt, 2)))
        e.set_proposal_prior_draw(0)
        e.init_from_prior()
        us = timed(e, n)
        out.append(us)
        print("polar D=%d %dx%d prior share %.2f, %s: %.2f us per PT step   [%s]" % (D, Nt, W, share, "polar + copolar dimensions" if trig else "all-uniform prior", us, e.step_kernel_name),
              flush=True)
        e.close()
    print("polar cost: %.2f us per PT step" % (out[1] - out[0]), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "population"
    a = sys.argv[2:]
    if mode == "population":
        population(int(a[0]) if a else 32, int(a[1]) if len(a) > 1 else 128, int(a[2]) if len(a) > 2 else 512, int(a[3]) if len(a) > 3 else 300)
    else:
        polar(int(a[0]) if a else 6, int(a[1]) if len(a) > 1 else 20, int(a[2]) if len(a) > 2 else 64, int(a[3]) if len(a) > 3 else 4000,
              float(a[4]) if len(a) > 4 else 0.1)
