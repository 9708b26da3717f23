"""Does the engine sample the right DISTRIBUTIONS where priors are not uniform, boundaries act, and the prior itself proposes?

The parity tests compare the kernels bit for bit with restatements written by the same hands; test_gpu_statistics.py samples one
target, a Gaussian in a box no chain ever touches.  Here every kernel family that carries general priors and boundaries, and the
prior-draw member in every place it can run, samples the "zoo" of tests/distribution_model.py -- `limit`, `reflect` and `wrap`
boundaries that act, Gaussian, polar, copolar and log priors, a diagonal Gaussian likelihood with a mean -- whose marginals of every
(rung, dimension) are known exactly (closed form or quadrature good to 1e-9, no engine and no checker in them).

Protocol of every case (the case tables are distribution_model.CASES_A / CASES_B, and CASES_C for differential evolution, whose
criterion is a covariance; tests/test_distribution_model_cpu.py holds every case to the design condition and runs those the CPU
checker can run through the same harness):
  * every chain of every rung starts from an exact inverse-cdf sample; S PT steps with swap_rate 0.2 (Metropolis moves and exchanges);
    S is at least 10 integrated autocorrelation times of the slowest (rung, dimension), written next to it in the table;
  * ONE snapshot at the end, independent ladders only: the counts in K = 16 equiprobable bins are exactly binomial under the null, no
    effective sample size is assumed; n >= 4096 per (rung, dimension); a family that takes fewer ladders per launch (the persistent
    ladder kernel) repeats the run on fresh engines with other seeds and pools the final snapshots;
  * acceptance: max |z| <= 5 over ALL rungs, dimensions and bins (at most 1008 of them: a false alarm has probability <= 6e-4; with
    fixed seeds the result is deterministic anyway); of evolving ladders, whose interior rungs have another temperature in every
    ladder, the cold rung alone -- with n = 16384, so that its alternatives are still rejected by 15 (prior_tempered is the truth at
    beta = 1 and no alternative there);
  * discrimination: the same counts reject every named wrong alternative of every dimension that has one by |z| >= 15 on at least one
    rung -- the committed proof that the case could fail (prior_twice is what a prior draw without its Hastings ratio converges to,
    prior_ignored / prior_tempered what a wrong tempering of the prior gives, untruncated what a boundary that does not act gives);
  * movement: 0.05 tries < accepted < 0.95 tries, exchanges were accepted, no chain's last_type is still -1;
  * the kernel is asserted by name."""
import os
import subprocess
import sys

if __name__ == "__main__":      # the device-likelihood case in a process of its own: python test_gpu_distributions.py "<case name>"
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch  # noqa: F401  (before anything loads the engine library: one HIP runtime per process)

import numpy as np
import pytest

import distribution_model as M
import prior_draw_model as PM
from ptmcmc_amd import engine as E
from distribution_util import covariance_error, de_inputs, de_rungs

pytestmark = pytest.mark.gpu


def _device_like(pb):
    """the same diagonal Gaussian in torch, on the engine's stream"""
    import torch
    mean = torch.as_tensor(pb.mean, dtype=torch.float64, device="cuda")
    inv = torch.as_tensor([1.0 / v.s for v in pb.dims], dtype=torch.float64, device="cuda")

    def fn(X, count, out):
        t = (X - mean) * inv
        out.copy_(-0.5 * (t * t).sum(dim=1))
    return fn


def make_engine(case, pb, seed, X0):
    """an engine on the case's problem, started from X0 [Nt][W][D]"""
    Nt, W = pb.Nt, case["W"]
    eng = E.Engine(pb.D, Nt, W, swap_rate=M.SWAP_RATE, seed=seed, **case["opts"])
    eng.set_bounds(*pb.bounds)
    eng.set_prior(*pb.prior)
    eng.set_target_gaussian(pb.precision, 0.0, pb.mean)
    if case["like"] == "host":      # the same diagonal Gaussian as a batched numpy callback: propose and accept passes around it
        eng.set_target_callback(pb.log_like, batched=True)
    if case["like"] == "device":
        eng.set_target_device(_device_like(pb))
    eng.set_ladder(pb.beta)
    if case["evolve"] > 0:
        eng.set_evolve_temps(case["evolve"])
    eng.set_proposals(E.PROP_DIAG, pb.proposal_sigmas(case["fac"]), np.full(Nt, case["oned"]))
    member = case["member"]
    if member == "alone":           # a set of the prior member alone
        eng.set_proposal_mixture(np.ones((Nt, 1)), np.ones((Nt, 1)), np.zeros((Nt, 1)))
        eng.set_proposal_prior_draw(0)
    elif member is not None:        # {Gaussian, prior}: (share of the prior member, Tpow); Tpow > 0: every rung its own table
        share, Tpow = member
        cum = np.array([PM.thermal_bins([1.0 - share, share], [0.0, 1.0], Tpow, float(b))[1] for b in pb.beta])
        cum[:, -1] = 1.0
        if Tpow > 0:
            assert cum[-1, 0] < cum[0, 0] - 0.3       # the prior's share grows towards the hot rungs
        eng.set_proposal_mixture(cum, np.ones((Nt, 2)), np.tile([case["oned"], 0.0], (Nt, 1)))
        eng.set_proposal_prior_draw(1)
    eng.set_states(X0.reshape(Nt * W, pb.D))
    return eng


def run_case(case):
    pb = M.problem_of(case)
    Nt, W, S = pb.Nt, case["W"], case["S"]
    snaps, tries, acc, sw_t, sw_a, stuck, types = [], 0, 0, 0, 0, 0, set()
    for k in range(case["runs"]):
        X0 = pb.exact_samples(W, np.random.default_rng(case["seed"] + k))
        eng = make_engine(case, pb, case["seed"] + k, X0)
        names = (eng.step_kernel_name, eng.sweep_kernel_name)
        assert any(case["kernel"] in v for v in names), (case["kernel"], names)
        eng.step(S); eng.sync()
        snaps.append(eng.states().reshape(Nt, W, pb.D))
        tries += int(eng.ntries.sum()) - eng.Nc; acc += int(eng.naccept.sum()) - eng.Nc
        t, a = eng.swap_counts()
        sw_t += int(t.sum()); sw_a += int(a.sum())
        lt = eng.last_type
        stuck += int((lt == -1).sum()); types |= set(int(v) for v in np.unique(lt))
        if "ladder_persistent_kernel" in case["kernel"]:
            st = eng.ladder_stats()
            assert st["launches"] > 0 and st["fallbacks"] == 0 and not st["disabled"], st
        eng.close()
    X = np.concatenate(snaps, axis=1)
    n = X.shape[1]
    assert n == W * case["runs"] >= 4096
    rungs, exclude = M.judged(case)      # (an evolving ladder: the cold rung alone, where prior_tempered is the truth and no alternative)
    c = pb.counts(X)
    z, where = M.worst_z(pb, c, n, rungs)
    rej = M.rejections(pb, c, n, rungs, exclude)
    weakest = min(rej, key=rej.get)
    print("%s: worst |z| = %.2f at (rung, dimension, bin) %s of %d bins judged, n = %d, acceptance %.3f, exchanges accepted %.3f, weakest "
          "rejection %.1f %s, type codes %s, kernel %s | %s" % (case["name"], z, where, c[rungs].size, n, acc / tries, sw_a / max(1, sw_t), rej[weakest],
                                                                 weakest, sorted(types), names[0], names[1]))
    assert z <= M.Z_BOUND, (z, where)
    assert rej[weakest] >= M.Z_REJECT, rej
    assert 0.05 * tries < acc < 0.95 * tries, (acc, tries)
    assert sw_a > 0 and stuck == 0, (sw_a, stuck)
    return types


@pytest.mark.parametrize("case", M.CASES_A, ids=[c["name"] for c in M.CASES_A])
def test_priors_and_bounds_under_gaussian_proposals(case):
    """cases A: one per kernel family that carries general priors and boundaries and fits the bin budget (distribution_model.CASES_A
    says which two do not, and why)"""
    run_case(case)


@pytest.mark.parametrize("case", M.CASES_B, ids=[c["name"] for c in M.CASES_B])
def test_the_prior_draw_member_with_the_likelihood_on(case):
    """cases B: the member alone (prior_twice is exactly what a missing or mis-priced Hastings ratio converges to; on the hot rungs
    most draws are accepted, so a wrong draw density -- the 64 bisections of polar and copolar, exp for log, Box-Muller for Gaussian --
    shows there), {Gaussian 0.7, prior 0.3} on the general and the lanes kernel, the same with thermal shares, and around a
    host-callback likelihood, whose accept pass finds member and ratio again"""
    if case["like"] == "device" and __name__ != "__main__":
        r = subprocess.run([sys.executable, os.path.abspath(__file__), case["name"]], capture_output=True, text=True, timeout=300)
        if r.returncode < 0 or r.returncode in (134, 139):   # a crashed child (abort, fault): start nothing more on the device
            pytest.exit("the device-likelihood case died (exit %d)\n%s" % (r.returncode, r.stderr[-6000:]), returncode=1)
        print(r.stdout[-2000:])
        assert r.returncode == 0 and "ok device likelihood" in r.stdout, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-6000:])
        return
    types = run_case(case)
    prior_code = 0 if case["member"] == "alone" else 1
    assert prior_code in types, types            # prior draws were accepted
    if case["member"] != "alone":
        assert types & {0, 10}, types            # ... and Gaussian moves beside them


@pytest.mark.parametrize("case", M.CASES_C, ids=[c["name"] for c in M.CASES_C])
def test_differential_evolution_with_many_snooker_moves(case):
    """cases C: snooker share 0.5 (the sampler's is 0.1), whose Hastings term is the Jacobian (r'/r)^(D-1), in every family that draws
    differential evolution.  Differential evolution from a chain's own history is adaptive and only asymptotically invariant: the
    checker's run of the same cases (test_distribution_model_cpu.py) shows that 0.5 is a fair null -- the reference's own rule stays
    inside the bound.  The colder half of the rungs is compared, as in test_gpu_statistics.py; of evolving ladders (the persistent
    kernel's build 15) the cold rung alone."""
    D, Nt, W, S = case["D"], case["Nt"], case["W"], case["S"]
    snaps, types, tries, acc, sw_a = [], set(), 0, 0, 0
    for k in range(case["runs"]):
        pr, cum, scales, odfs, cap, init, X0 = de_inputs(case, k)
        eng = E.Engine(D, Nt, W, swap_rate=M.SWAP_RATE, add_every_n=M.DE_EVERY, history_rungs=Nt, history_capacity=cap, seed=case["seed"] + k, **case["opts"])
        pr.configure(eng, E.PROP_DIAG)
        eng.set_proposal_mixture(cum, scales, odfs)
        eng.set_proposal_de(M.DE_SNOOKER, 0.3, 4.0, 0.0, init_rows=init)
        if case["evolve"] > 0:
            eng.set_evolve_temps(case["evolve"])
        eng.set_states(X0.reshape(Nt * W, D))
        names = (eng.step_kernel_name, eng.sweep_kernel_name)
        assert any(case["kernel"] in v for v in names), (case["kernel"], names)
        eng.step(S); eng.sync()
        snaps.append(eng.states().reshape(Nt, W, D))
        types |= set(int(v) for v in np.unique(eng.last_type))
        tries += int(eng.ntries.sum()) - eng.Nc; acc += int(eng.naccept.sum()) - eng.Nc
        sw_a += int(eng.swap_counts()[1].sum())
        if "ladder_persistent_kernel" in case["kernel"]:
            st = eng.ladder_stats()
            assert st["launches"] > 0 and st["fallbacks"] == 0 and not st["disabled"], st
        eng.close()
    X = np.concatenate(snaps, axis=1)
    n = X.shape[1]
    assert n == W * case["runs"] >= 4096
    bound = 5.0 * np.sqrt(2.0 / n)
    err = covariance_error(pr, X, de_rungs(case))
    print("differential evolution, snooker %.1f, %s: max |C - cov / beta| / (sigma_i sigma_j) = %.4f over rungs %s (bound %.4f, n = %d), acceptance %.3f, type "
          "codes %s, kernel %s | %s" % (M.DE_SNOOKER, case["name"], err, de_rungs(case), bound, n, acc / tries, sorted(types), names[0], names[1]))
    assert err < bound, (err, bound)
    assert 0.05 * tries < acc < 0.95 * tries and sw_a > 0 and -1 not in types
    assert types & {0, 10}, types          # differential-evolution moves were accepted


if __name__ == "__main__":
    case = [c for c in M.CASES_B if c["name"] == sys.argv[1]][0]
    test_the_prior_draw_member_with_the_likelihood_on(case)
    print("ok device likelihood")
