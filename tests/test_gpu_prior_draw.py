"""Independent draws from the prior as a member of the proposal set, drawn ON THE DEVICE (ptm_set_proposal_prior_draw), against
tests/prior_draw_model.py, which restates the move from the CPU oracle's primitives and steps the frozen oracle through it.  Bit for
bit: states, likelihoods, priors, counters, type codes, every saved row and the MAP -- on the general kernel, the lanes kernel and both
adaptive builds, with differential evolution beside it, under user likelihoods, on rung shards; and one property no model is needed for."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import adaptive_model as AM
import oracle_lib as O
import parity_util as PU
import prior_draw_cases as PC
import prior_draw_model as PM
from ptmcmc_amd import engine as E
from proposal_pairs import doubling as _doubling

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED = PC.SEED
ERR_INVALID, ERR_UNSUPPORTED = -1, -2   # ptm_status (include/ptm_engine.h)


def _child(case, env=None, timeout=300):
    """a case in a process of its own (an environment switch the engine reads once, or torch imported first)"""
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(HERE, "prior_draw_cases.py"), case], capture_output=True, text=True, timeout=timeout, env=e)
    if r.returncode < 0 or r.returncode in (134, 139):   # a crashed child (abort, fault): start nothing more on the device
        pytest.exit("prior-draw case %s died (exit %d)\n%s" % (case, r.returncode, r.stderr[-6000:]), returncode=1)
    assert r.returncode == 0 and ("ok " + case) in r.stdout, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-6000:])


def test_general_kernel_ragged_population():
    """D = 3, 4 rungs x 3 walkers, {Gaussian, prior, Gaussian}, uniform prior with `limit` bounds: sweep_kernel<4, 2, false, false>"""
    _child("ragged_general", {"PTM_FORCE_VALU": "1"})


def test_general_kernel_whole_waves_with_every_prior_type():
    """D = 5, 3 rungs x 64 walkers, evolving ladder; uniform, Gaussian, polar, copolar and log dimensions (the prior of
    test_init_from_prior_draws_every_support_type), a reflecting and a wrapping boundary inside the supports (the reflection
    one-sided: the reference's two-sided fold is not idempotent, and the checker enforces the start states it is handed once more)"""
    D, Nt, W, steps = 5, 3, 64, 40
    cap = 2 * steps + 8
    pi = math.pi
    prior = ([1, 2, 3, 4, 5], [0.5, 0.3, pi / 2, 0.1, 3.0], [2.0, 1.5, pi / 2 - 0.2, 1.2, 2.5])
    blo = [E.BOUND_REFLECT, E.BOUND_OPEN, E.BOUND_OPEN, E.BOUND_WRAP, E.BOUND_OPEN]
    bhi = [E.BOUND_OPEN, E.BOUND_OPEN, E.BOUND_OPEN, E.BOUND_WRAP, E.BOUND_OPEN]
    bounds = (blo, bhi, [-1.2, 0.0, 0.0, -1.0, 0.0], [0.0, 0.0, 0.0, 1.2, 0.0])
    pr, eng, lad, model = PC.mixture_pair(D, Nt, W, E.PROP_DIAG, PC.cum_of([0.3, 0.4, 0.3]), [1.0, 1.0, 0.25], [0.5, 0.0, 0.0], 1, cap=cap,
                                          evolve=0.01, prior=prior, bounds=bounds)
    assert eng.sweep_kernel_name == "sweep_kernel<8, 1, true, false>", eng.sweep_kernel_name
    assert eng.step_kernel_name.startswith("decide_kernel + sweep_kernel<"), eng.step_kernel_name
    PC.run(eng, lad, model, steps)
    assert np.array_equal(eng.invtemps(), lad.betaw)
    PC.assert_same_history(eng, lad, model, cap)
    PC.check_member_was_used(eng, model, 1)
    eng.close()


@pytest.mark.parametrize("D,Nt,W,kernel", [(21, 4, 2, "sweep_lanes_kernel<32, 2, true>"), (40, 2, 2, "sweep_lanes_kernel<64, 2, true>")])
def test_lanes_kernel_with_a_gaussian_prior(D, Nt, W, kernel):
    """a lane per dimension draws its dimension: 21 of 32 lanes, and 40 of 64 (a wave per chain)"""
    steps = 40
    cap = 2 * steps + 8
    pr0 = PU.problem_for(D, Nt, 1e3)
    prior = ([E.PRIOR_GAUSSIAN] * D, np.zeros(D), 1.5 * np.sqrt(np.diag(pr0.cov)))
    pr, eng, lad, model = PC.mixture_pair(D, Nt, W, E.PROP_LOWER, PC.cum_of([0.3, 0.4, 0.3]), [1.0, 1.0, 0.25], [0.5, 0.0, 0.0], 1, cap=cap, prior=prior)
    assert eng.sweep_kernel_name == kernel, eng.sweep_kernel_name
    PC.run(eng, lad, model, steps)
    PC.assert_same_history(eng, lad, model, cap)
    assert model.moves.sum() > 0
    eng.close()


@pytest.mark.parametrize("W,kernel", [(3, "sweep_lanes_kernel<4, 1, true>"), (64, "sweep_kernel<4, 1, true, false>")])
def test_with_differential_evolution_and_the_hand_over(W, kernel):
    """{differential evolution, prior, Gaussian}, D = 3, no initial rows: until 30 rows are saved differential evolution is not ready
    and its pick lands on the prior member behind it; then it is drawn from the history the prior draws helped to fill"""
    D, Nt, steps = 3, 4, 45
    cap = 2 * steps + 8
    pr, eng, lad, model = PC.mixture_pair(D, Nt, W, E.PROP_DIAG, PC.cum_of([0.5, 0.2, 0.3]), [-1.0, 1.0, 0.5], [0.0, 0.0, 0.5], 1, cap=cap, de=0.2)
    assert eng.sweep_kernel_name == kernel, eng.sweep_kernel_name
    assert "persistent" not in eng.step_kernel_name and "ladder_steps" not in eng.step_kernel_name, eng.step_kernel_name
    eng.step(12); eng.sync(); model.step(12)          # (at most two saved rows per step: no chain has 30 yet)
    PC.assert_same(eng, lad, model, "after 12 steps")
    # nothing but the prior member and the Gaussian so far, and the prior member with differential evolution's share on top of its own
    # (0.5 + 0.2 of the moves expected; below 0.5 is more than four standard deviations of the smaller population's count away)
    assert set(int(v) for v in np.unique(eng.last_type)) <= {-1, 1, 2, 12}
    assert model.moves.sum() > 0.5 * (eng.ntries.sum() - eng.Nc)
    eng.step(33); eng.sync(); model.step(33)
    PC.assert_same(eng, lad, model, "after 45 steps")
    PC.assert_same_history(eng, lad, model, cap)
    he = eng.history()
    seen = set(int(v) for row in he["last_type"][:int(eng.nsize.min())] for v in np.unique(row))
    assert (0 in seen or 10 in seen) and 1 in seen, seen
    eng.close()


def test_host_callback_likelihood():
    """the propose and accept passes around a host likelihood: the accept pass finds member and ratio again"""
    c, k = [0.3, -0.2, 0.5], [-1.0, -2.5, -0.6]
    f = PC.quad_host(c, k)
    eng, lad, model = PC.user_like_pair(lambda e: e.set_target_callback(f), f)
    assert eng.sweep_kernel_name == "sweep_lanes_kernel<4, 1, true>", eng.sweep_kernel_name
    PC.run(eng, lad, model, 40)
    PC.check_member_was_used(eng, model, 1)
    eng.close()


def test_device_likelihood():
    """... and around a torch likelihood on the device (a process that imports torch first)"""
    _child("device_like")


@pytest.mark.parametrize("Nt,W,kernel", [(3, 2, "sweep_lanes_ada_kernel<4, 1>"), (2, 64, "sweep_kernel<4, 1, true, false, true>")])
def test_adaptive_set_with_thermal_top_thresholds(Nt, W, kernel):
    """{differential evolution, prior, nested set of three Gaussians adapting at 0.05}, top rate 0 with every rung's thermal thresholds
    (the sampler's --prior_draw_frac --prior_draw_Tpow --prop_adapt_rate): they enter the initial state and are never rebuilt"""
    D, steps = 3, 45
    cap = 2 * steps + 8
    pr0 = PU.problem_for(D, Nt, 1e3)
    pr, eng, lad = PU.make_pair(D, Nt, W, 1e3, kind=E.PROP_DIAG, seed=SEED, swap_rate=0.3, history_cap=cap, prior=PC.box_prior(pr0))
    top, hot, Tpow, inner = [0.5, 0.2, 0.3], [0.0, 1.0, 0.0], 0.3, _doubling(3)   # (a mild power: the hot rungs keep some of every member)
    scales, odfs = [-1.0, 1.0, 1.0, 1.0, 0.5, 0.25], [0.0, 0.0, 0.0, 0.5, 0.5, 0.5]
    chains = [PM.thermal_chain_set(top, hot, Tpow, float(pr.beta[r]), 2, inner, 0.05) for r in range(Nt) for _ in range(W)]
    assert chains[-1].top.bin_max != chains[0].top.bin_max
    w, th, bits, cnt = AM.states_of(chains)
    sc, od = np.tile(scales, (Nt, 1)), np.tile(odfs, (Nt, 1))
    eng.set_proposal_adaptive(3, sc, od, w, th, bits, cnt, nested=2, K_inner=3, rate=0.0, rate_inner=0.05)
    eng.set_proposal_prior_draw(1)
    eng.set_proposal_de(0.2, 0.3, 4.0, 0.0); lad.set_de(0.2, 0.3, 4.0, 0.0)
    model = PM.PriorDrawOracle(lad, SEED, chains, sc, od, 1)
    assert eng.sweep_kernel_name == kernel, eng.sweep_kernel_name
    PC.run(eng, lad, model, steps, adaptive=True)
    PC.assert_same_history(eng, lad, model, cap)
    PC.check_member_was_used(eng, model, 1)
    st = eng.proposal_adapt_state()
    assert np.array_equal(st["thresholds"][:, :3], th[:, :3]) and not st["outcomes"][:, 0].any() and st["outcomes"][:, 1].max() > 0
    eng.close()


def test_every_prior_draw_under_a_flat_likelihood_is_accepted():
    """No model: a set of the prior member alone, likelihood identically 0, uniform + polar + log prior, open bounds.  Then
    logH = (lp - nlp) + (nlp - lp) = 0 exactly, so every move of a rung the exchange phase left alone is accepted: naccept rises by
    exactly the number of Metropolis moves (the rise of ntries), and every state lies in the support."""
    D, Nt, W, steps = 3, 4, 3, 40
    pi = math.pi
    types, cen, hw = [E.PRIOR_UNIFORM, E.PRIOR_POLAR, E.PRIOR_LOG], [0.5, pi / 2, 3.0], [2.0, pi / 2 - 0.2, 2.5]
    eng = E.Engine(D, Nt, W, swap_rate=0.3, seed=SEED)
    eng.set_bounds([E.BOUND_OPEN] * D, [E.BOUND_OPEN] * D, np.zeros(D), np.zeros(D))
    eng.set_prior(types, cen, hw)
    eng.set_target_gaussian(np.zeros((D, D)), 0.0)
    eng.set_ladder(E.geometric_ladder(Nt, 1e2))
    eng.set_proposals(E.PROP_DIAG, np.full((Nt, D), 0.1))
    eng.set_proposal_mixture(np.ones((Nt, 1)), np.ones((Nt, 1)), np.zeros((Nt, 1)))
    eng.set_proposal_prior_draw(0)
    eng.init_from_prior()
    assert not (eng.llike != 0.0).any()
    x0, nt0, na0 = eng.states(), eng.ntries.copy(), eng.naccept.copy()
    assert "persistent" not in eng.step_kernel_name and "ladder_steps" not in eng.step_kernel_name, eng.step_kernel_name
    eng.step(steps); eng.sync()
    moves = eng.ntries - nt0
    assert moves.min() > 0 and moves.sum() < steps * eng.Nc        # (some steps went to the exchange phase)
    assert np.array_equal(eng.naccept - na0, moves)
    x = eng.states()
    assert not np.array_equal(x, x0)
    lo = [cen[0] - hw[0], cen[1] - hw[1], cen[2] / hw[2]]
    hi = [cen[0] + hw[0], cen[1] + hw[1], cen[2] * hw[2]]
    for d in range(D):
        assert (x[:, d] >= lo[d]).all() and (x[:, d] <= hi[d]).all(), d
    assert np.isfinite(eng.lprior).all() and set(int(v) for v in np.unique(eng.last_type)) == {0}
    eng.close()


def test_two_rung_shards_equal_one_engine():
    """3 + 3 rungs in two engines of one process, stepped in the overlapped order (partial sweeps: ptm_sweep_rungs) = one engine of 6:
    the streams are keyed by the global rung"""
    import shard_sim
    from ptmcmc_amd.parallel import shard_bounds
    from test_gpu_parity import _DevShard
    D, Nt, W, steps = 5, 6, 4, 40
    pr = PU.problem_for(D, Nt, 1e3)
    prior = PC.box_prior(pr)
    cum, scales, odfs = np.tile(PC.cum_of([0.3, 0.4, 0.3]), (Nt, 1)), np.tile([1.0, 1.0, 0.25], (Nt, 1)), np.tile([0.5, 0.0, 0.0], (Nt, 1))
    cum[:, 1] = np.linspace(0.5, 0.9, Nt)     # (a table per rung: each shard gets its own rows)

    def setup(e, r0, n):
        pr.configure(e, E.PROP_LOWER)
        e.set_prior(*prior)
        e.set_proposal_mixture(cum[r0:r0 + n], scales[r0:r0 + n], odfs[r0:r0 + n])
        e.set_proposal_prior_draw(1)
    ref = E.Engine(D, Nt, W, swap_rate=0.3, seed=SEED)
    setup(ref, 0, Nt)
    ref.init_from_prior()
    x0 = ref.states()
    shards = []
    for g in range(2):
        r0, n = shard_bounds(Nt, 2, g)
        e = E.Engine(D, Nt, W, swap_rate=0.3, seed=SEED, rung_begin=r0, rung_count=n)
        setup(e, r0, n)
        e.set_states(x0[r0 * W:(r0 + n) * W])
        shards.append(e)
    lads = shard_sim.build([_DevShard(e) for e in shards], halo=4, recover=True)   # (a halo of 3 rungs at most: long runs of picks are recovered)
    copy = lambda dst, src: dst.copy_from(src.ptr, min(dst.nbytes, src.nbytes))
    ref.step(steps); ref.sync()
    shard_sim.step_overlapped(lads, copy, steps)
    for e in shards:
        e.sync()
    for name in ("states", "llike", "lprior", "naccept", "ntries", "last_type"):
        got = np.concatenate([getattr(e, name)() if name == "states" else getattr(e, name) for e in shards])
        want = ref.states() if name == "states" else getattr(ref, name)
        assert np.array_equal(got, want), name
    assert 1 in set(int(v) for v in np.unique(ref.last_type))
    for e in shards + [ref]:
        e.close()


def test_refusals_leave_the_member_working_and_routing():
    D, Nt, W = 3, 4, 3
    pr, eng, lad, model = PC.mixture_pair(D, Nt, W, E.PROP_DIAG, PC.cum_of([0.5, 0.2, 0.3]), [-1.0, 1.0, 0.5], [0.0, 0.0, 0.5], 1, cap=64, de=0.2)
    PC.run(eng, lad, model, 10, chunks=(1,))
    L = eng.L
    for member in (3, -2, 17):                       # out of range
        assert L.ptm_set_proposal_prior_draw(eng.h, member) == ERR_INVALID, member
    assert L.ptm_set_proposal_prior_draw(eng.h, 0) == ERR_INVALID          # the differential-evolution member
    assert b"differential evolution" in L.ptm_last_error()
    with pytest.raises(E.PtmError):
        eng.set_proposal_prior_draw(5)
    PC.run(eng, lad, model, 6, chunks=(1,))           # the member named before still draws
    PC.check_member_was_used(eng, model, 1)
    eng.close()
    # unsupported: a flat prior dimension; a prior callback
    pr = PU.problem_for(D, Nt, 1e3)
    eng = E.Engine(D, Nt, W)
    pr.configure(eng, E.PROP_DIAG)
    tab = (np.tile([0.5, 1.0], (Nt, 1)), np.ones((Nt, 2)), np.zeros((Nt, 2)))
    assert eng.L.ptm_set_proposal_prior_draw(eng.h, 0) == ERR_INVALID      # no set yet
    eng.set_proposal_mixture(*tab)
    eng.set_prior([E.PRIOR_UNIFORM, E.PRIOR_FLAT, E.PRIOR_UNIFORM], pr.centers, pr.halfwidths)
    assert eng.L.ptm_set_proposal_prior_draw(eng.h, 0) == ERR_UNSUPPORTED and b"flat" in eng.L.ptm_last_error()
    eng.set_prior(pr.types, pr.centers, pr.halfwidths)
    eng.set_proposal_prior_draw(0)
    eng.set_proposal_prior_draw(-1)                   # off again
    eng.set_prior_callback(lambda x: 0.0)
    assert eng.L.ptm_set_proposal_prior_draw(eng.h, 0) == ERR_UNSUPPORTED and b"prior" in eng.L.ptm_last_error()
    eng.close()
    # routing: 32 dimensions, whole waves per rung: no matrix cores; a short ladder of one walker: neither the persistent nor the fused kernel
    # (without the member: the sweep of such a 32-dimensional population is the matrix-core kernel's, its step and the short ladder's the
    #  persistent kernel's)
    for D_, Nt_, W_, before in ((32, 2, 64, "sweep_mfma32"), (4, 4, 1, "ladder_")):
        pr, eng, lad = PU.make_pair(D_, Nt_, W_, 1e3, kind=E.PROP_DIAG, seed=SEED)
        eng.set_proposal_mixture(np.tile([0.5, 1.0], (Nt_, 1)), np.ones((Nt_, 2)), np.zeros((Nt_, 2)))
        names = lambda: eng.sweep_kernel_name + " | " + eng.step_kernel_name
        assert before in names() and "ladder_" in eng.step_kernel_name, names()
        eng.set_proposal_prior_draw(1)
        name = names()
        assert "sweep_mfma32" not in name and "ladder_persistent_kernel" not in name and "ladder_steps_kernel" not in name, name
        step = eng.step_kernel_name
        assert step.startswith("decide_kernel + sweep_lanes_kernel<") or step.startswith("decide_kernel + sweep_kernel<"), step
        eng.step(5); eng.sync()
        eng.set_proposal_prior_draw(-1)
        assert before in names(), names()
        eng.close()


_FACADE = r'''
#include <cstdio>
#include <string>
#include <vector>
#include "ptmcmc_gpu.hh"
using namespace ptmgpu;
int main(int argc, char** argv) {
  const int D = 3;
  std::vector<double> P = {2.0, 0.6, 0.0, 0.6, 1.0, -0.3, 0.0, -0.3, 1.5};
  stateSpace space(D);
  std::vector<std::string> names = {"a", "b", "c"};
  space.set_names(names);
  gaussian_likelihood like(P, 0.0);
  std::vector<std::string> types(D, "uni");
  std::vector<double> centers(D, 0.0), scales(D, 4.0);
  like.basic_setup(&space, types, centers, scales);
  ptmcmc_sampler mcmc;
  mcmc.set("nsteps", "300"); mcmc.set("pt", "6"); mcmc.set("pt_Tmax", "50"); mcmc.set("save_every", "1");
  mcmc.set("nevery", "100"); mcmc.set("nskip", "1"); mcmc.set("pt_dump_n", "6"); mcmc.set("pt_swap_rate", "0.3");
  if (!mcmc.parse(argc - 1, argv + 1)) { printf("bad option\n"); return 2; }
  mcmc.setup(like);
  mcmc.select_proposal();
  mcmc.initialize();
  mcmc.run(argv[1]);
  printf("host=%d prior_dev=%d\n", mcmc.chains()->proposals_on_host() ? 1 : 0, mcmc.chains()->draws_prior_on_device() ? 1 : 0);
  printf("step kernel: %s\n", ptm_step_kernel_name(mcmc.chains()->engine()));
  return 0;
}
'''


def test_the_samplers_recipe_draws_the_prior_on_the_device():
    """--prior_draw_frac=0.2 --prior_draw_Tpow=1 --pt=6, 300 steps through the facade's sampler: the device path by default, the
    host-proposal path under PTM_HOST_PRIOR_DRAW=1; both finish and the chain files carry the prior member's type code (member 1
    behind differential evolution).  The two paths use different random streams: the files are not compared."""
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.cc"), os.path.join(d, "t")
        open(src, "w").write(_FACADE)
        r = subprocess.run(["g++", "-std=c++11", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), src,
                            "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine", "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        for where in ("device", "host"):
            env = dict(os.environ)
            env.pop("PTM_HOST_PRIOR_DRAW", None)
            if where == "host":
                env["PTM_HOST_PRIOR_DRAW"] = "1"
            base = os.path.join(d, where)
            out = subprocess.run([exe, base, "--prior_draw_frac=0.2", "--prior_draw_Tpow=1", "--pt=6"], capture_output=True, text=True, timeout=300, env=env)
            if out.returncode < 0 or out.returncode in (134, 139):
                pytest.exit("the sampler died on the %s path (exit %d)\n%s" % (where, out.returncode, out.stderr[-4000:]), returncode=1)
            assert out.returncode == 0, (where, out.stdout[-3000:], out.stderr[-3000:])
            assert "Finished running chain" in out.stdout
            assert ("draws from the prior are made on the " + where) in out.stdout, out.stdout[-3000:]
            assert ("host=%d prior_dev=%d" % ((0, 1) if where == "device" else (1, 0))) in out.stdout, out.stdout[-2000:]
            if where == "device":
                assert "sweep_lanes_kernel<" in out.stdout or "sweep_kernel<" in out.stdout, out.stdout[-2000:]
            types = set()
            for k in range(6):
                for line in open("%s_t%d.dat" % (base, k)):
                    f = line.split()
                    if len(f) > 4 and not line.startswith("#"):
                        types.add(int(f[4].rstrip(":")))   # "step lpost llike acceptance type: parameters ..."
            assert 1 in types, (where, sorted(types))
