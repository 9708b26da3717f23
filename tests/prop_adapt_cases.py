"""The install cases of tests/test_gpu_prop_adapt.py: engine A adapts its proposals on the device (ptm_adapt_proposals); engine B, with
the same seeds and inputs, is handed A's factors_out through ptm_set_proposal_rung for the rungs of status 0; then both run on and must
stay identical in everything.  One case per install target that an engine with a history ring can reach.  plan_sweep
(ptmcmc_amd/csrc/ptm_sweep_plan.hpp) keeps such an engine off the 64- and 128-padded matrix-core kernels, off the compacted sweep and
with it off the box pre-pass (`!f.tracked`): at 61 and 125 dimensions the lanes kernels run, and the cases assert that -- the tiles and
the pre-pass's sigmas and margins are still installed, by the packer ptm_set_proposal_rung shares, for the day a kernel reads them.
usage: python prop_adapt_cases.py <case>"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prop_adapt_model as P
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem

# name: D, rungs, walkers, kind, warm-up steps, nrows, what the sweep kernel's name must contain, options
CASES = {
    "lanes": (6, 4, 3, E.PROP_DENSE, 60, 40, "sweep_lanes_kernel<8,", {}),
    "mfma32": (21, 2, 320, E.PROP_DENSE, 6, 4, "sweep_mfma32_kernel<0,", {}),
    "dim61": (61, 2, 64, E.PROP_DENSE, 6, 4, "sweep_lanes_kernel<64, 0,", {}),
    "dim125": (125, 2, 64, E.PROP_DENSE, 6, 4, "sweep_lanes_kernel<128, 0,", {"twin": False}),
    "ladder": (20, 7, 3, E.PROP_DENSE, 80, 30, "sweep_lanes_kernel<32,", {"step_name": "ladder_persistent_kernel<32,", "add": 2}),
    "big_diag": (21, 2, 1024, E.PROP_DIAG, 6, 3, "sweep_mfma32_kernel<2,", {"no_prefilter": True}),
    "diag6": (6, 4, 3, E.PROP_DIAG, 60, 40, "sweep_lanes_kernel<8, 1,", {}),
    "diag200": (200, 2, 5, E.PROP_DIAG, 12, 8, "sweep_lanes_kernel<256, 1,", {"tmax": 1e2}),
    "mixture_de": (6, 4, 64, E.PROP_DENSE, 12, 8, "sweep_kernel<8,", {"de": True}),
}
SEED = 0x5EEDAD01


def make(name):
    D, Nt, W, kind, warm, nrows, _, opt = CASES[name]
    eng = E.Engine(D, Nt, W, seed=SEED, swap_rate=0.3, add_every_n=opt.get("add", 1), history_rungs=Nt, history_capacity=warm + 16, map_rungs=Nt if opt.get("de") else 0)
    import parity_util as PU
    PU.problem_for(D, Nt, 1e2).configure(eng, kind)
    if opt.get("de"):                                  # the sampler's mixture: a Gaussian member, its half-scale copy, differential evolution
        eng.set_proposal_mixture(np.tile([0.4, 0.7, 1.0], (Nt, 1)), np.tile([1.0, 0.5, -1.0], (Nt, 1)), np.zeros((Nt, 3)))
        init = np.random.default_rng(5).uniform(-1.0, 1.0, size=(4, Nt * W, D))      # rows in front of the start state for the first draws
        eng.set_proposal_de(0.1, 0.3, 4.0, 0.0, init_rows=init)
    eng.init_from_prior()
    return eng


def everything(eng):
    eng.sync()
    h = eng.history()
    out = dict(x=eng.states(), llike=eng.llike, lprior=eng.lprior, ntries=eng.ntries, naccept=eng.naccept, last_type=eng.last_type, nhist=eng.nhist,
               swap_tries=eng.swap_counts()[0], swap_accepts=eng.swap_counts()[1], last_pairs=eng.last_swaps()[0], last_accepts=eng.last_swaps()[1])
    held = h["row"] >= 0                               # (a slot nothing was saved in yet holds whatever the allocation held)
    for k, v in h.items():
        v = np.array(v)
        v[~held] = 0
        out["hist_" + k] = v
    return out


def assert_identical(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def run_on(eng):
    eng.step(3)
    eng.sweep(2)
    eng.step(2)


def run_case(name):
    D, Nt, W, kind, warm, nrows, sweep_name, opt = CASES[name]
    diag = kind == E.PROP_DIAG
    A, B = make(name), make(name)
    try:
        assert sweep_name in A.sweep_kernel_name, (name, A.sweep_kernel_name)
        if opt.get("step_name"):
            assert opt["step_name"] in A.step_kernel_name, (name, A.step_kernel_name)
        if opt.get("no_prefilter"):                    # a big population with history is not compacted: the box pre-pass never runs
            assert not A.prefilter_counts()["eligible"], name
        for e in (A, B):
            e.step(warm)
        assert_identical(everything(A), everything(B), (name, "before"))
        scale = 2.38 / np.sqrt(D)
        mean, cov, var, N = A.moments_rungs(nrows=nrows)
        assert N == W * nrows and mean.shape == (Nt, D)
        status, fac = A.adapt_proposals(nrows=nrows, factors=True)
        assert (status == 0).any(), (name, status)
        for r in range(Nt):
            if diag:
                want, st = P.adapt(var[r], scale, diag=True)
            elif opt.get("twin", True) or r == 0:
                want, st = P.adapt(cov[r], scale)
            else:      # (the twin takes seconds a rung here: it checks rung 0; the others: ptm_eigen_factors, held to the twin by its own test)
                F, lam = E.eigen_factors(cov[r], lambdas=True)
                want, st = np.float64(scale) * F, P.dense_status(cov[r], lam)
            assert status[r] == st, (name, r, status[r], st)
            assert P.same_bits(fac[r], want), (name, r)
            if st == 0:
                B.set_proposal_rung(r, fac[r])
        for e in (A, B):
            run_on(e)
        assert_identical(everything(A), everything(B), (name, "after"))
        assert (A.naccept != A.ntries).any()
        # the default arguments: 2.38 / sqrt(D), the largest common window
        s2 = A.adapt_proposals()
        assert s2.shape == (Nt,) and s2.dtype == np.int32
    finally:
        A.close()
        B.close()
    return "ok %s status=%s" % (name, "".join(str(int(s)) for s in status))


if __name__ == "__main__":
    print(run_case(sys.argv[1]))
