"""Engine-and-model pairs of the prior-draw tests (tests/test_gpu_prior_draw.py) and the comparison they share.  A case whose kernel needs
an environment switch of the engine (read once per process) runs in a process of its own:
    python prior_draw_cases.py ragged_general"""
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ["device_like"]:
        import torch  # noqa: F401  (before anything loads the engine library: one HIP runtime per process)

import adaptive_model as AM
import oracle_lib as O
import parity_util as PU
import prior_draw_model as PM
from ptmcmc_amd import engine as E

SEED = 0x5EED0001


def cum_of(shares):
    s = np.cumsum(np.asarray(shares, dtype=np.float64) / np.sum(shares))
    s[-1] = 1.0
    return s


def box_prior(pr, sigmas=3.0):
    """a uniform prior of a few sigma of the target: prior draws are accepted often enough to matter"""
    D = pr.D
    return ([E.PRIOR_UNIFORM] * D, np.zeros(D), sigmas * np.sqrt(np.diag(pr.cov)))


def mixture_pair(D, Nt, W, kind, cum, scales, odfs, member, cap=0, de=None, evolve=0.0, swap_rate=0.3, prior=None, bounds=None, sigmas=3.0):
    """a fixed set (one table for all rungs, or [Nt][K]) with member `member` drawing from the prior, and its model"""
    pr0 = PU.problem_for(D, Nt, 1e3)
    if prior is None:
        prior = box_prior(pr0, sigmas)
    pr, eng, lad = PU.make_pair(D, Nt, W, 1e3, kind=kind, seed=SEED, swap_rate=swap_rate, history_cap=cap, prior=prior, bounds=bounds)
    cum = np.asarray(cum, dtype=np.float64)
    C_ = np.tile(cum, (Nt, 1)) if cum.ndim == 1 else cum
    S_, O_ = np.tile(scales, (Nt, 1)), np.tile(odfs, (Nt, 1))
    eng.set_proposal_mixture(C_, S_, O_)
    eng.set_proposal_prior_draw(member)
    if de is not None:
        eng.set_proposal_de(de, 0.3, 4.0, 0.0)
        lad.set_de(de, 0.3, 4.0, 0.0)
    if evolve:
        eng.set_evolve_temps(evolve); lad.evolve_temps(evolve)
    chains = [PM.FixedSet(C_[r]) for r in range(Nt) for _ in range(W)]
    model = PM.PriorDrawOracle(lad, SEED, chains, S_, O_, member)
    return pr, eng, lad, model


def assert_same(eng, lad, model, what, adaptive=False):
    Nt, W = eng.Nt, eng.W
    xe, xo = eng.states(), PU.to_engine_order(lad.x, Nt, W)
    assert np.array_equal(xe, xo), "%s: states differ at %s" % (what, np.argwhere(xe != xo)[:4].tolist())
    for name in ("llike", "lprior", "ntries", "naccept", "nhist", "nsize"):
        a, b = getattr(eng, name), PU.to_engine_order(getattr(lad, name), Nt, W)
        assert np.array_equal(a, b), "%s: %s differ at %s" % (what, name, np.argwhere(a != b)[:4].tolist())
    lt = model.last_type()
    assert np.array_equal(eng.last_type, lt), "%s: last_type differ at %s" % (what, np.argwhere(eng.last_type != lt)[:4].tolist())
    if adaptive:
        st = eng.proposal_adapt_state()
        w, th, bits, cnt = model.state()
        for name, got, want in (("weights", st["weights"], w), ("thresholds", st["thresholds"], th), ("repeat bits", st["repeat_bits"], bits),
                                ("outcomes", st["outcomes"], cnt)):
            assert np.array_equal(got, want), "%s: adaptive %s differ at %s" % (what, name, np.argwhere(got != want)[:4].tolist())


def assert_same_history(eng, lad, model, cap):
    """every saved row and every rung's MAP (type codes through the model's mapping)"""
    Nt, W = eng.Nt, eng.W
    he, ho = eng.history(), lad.history()
    nsize = eng.nsize
    assert nsize.max() <= cap
    for name in ("x", "llike", "lprior", "naccept", "ntries", "last_type", "invtemp"):
        for s_ in range(int(nsize.max())):
            have = nsize > s_
            want = PU.to_engine_order(ho[name][:, s_], Nt, W)
            if name == "last_type":
                want = np.array([AM.nested_type(v, model.K, model.nested) for v in want])
            got = he[name][s_ % cap][have]
            assert np.array_equal(got, want[have]), (name, s_)
    m = eng.map()
    assert np.array_equal(m["lpost"], PU.to_engine_order(lad.map_lpost, Nt, W))
    assert np.array_equal(m["x"], PU.to_engine_order(lad.map_x, Nt, W))


def run(eng, lad, model, steps, chunks=(1, 6), adaptive=False):
    done = 0
    for n in list(chunks) + [steps - sum(chunks)]:
        eng.step(n); eng.sync(); model.step(n)
        done += n
        assert_same(eng, lad, model, "after %d steps" % done, adaptive)


def check_member_was_used(eng, model, member):
    """the prior member proposed, and some of its proposals were accepted (its type code, member + 10 * 0, is on record)"""
    assert model.moves.sum() > 0
    assert member in set(int(v) for v in np.unique(eng.last_type)), np.unique(eng.last_type)


def ragged_general():
    """D = 3 (one padded lane), 4 rungs x 3 walkers on the general kernel (PTM_FORCE_VALU=1), set {Gaussian, prior, Gaussian}, uniform
    prior with `limit` bounds inside it: some draws leave the bounds and are invalid"""
    D, Nt, W, steps = 3, 4, 3, 40
    cap = 2 * steps + 8
    pr0 = PU.problem_for(D, Nt, 1e3)
    s = np.sqrt(np.diag(pr0.cov))
    bounds = ([E.BOUND_LIMIT] * D, [E.BOUND_LIMIT] * D, -2.5 * s, 2.5 * s)
    pr, eng, lad, model = mixture_pair(D, Nt, W, E.PROP_LOWER, cum_of([0.3, 0.4, 0.3]), [1.0, 1.0, 0.25], [0.5, 0.0, 0.0], 1, cap=cap, bounds=bounds)
    assert eng.sweep_kernel_name == "sweep_kernel<4, 2, false, false>", eng.sweep_kernel_name
    run(eng, lad, model, steps)
    assert_same_history(eng, lad, model, cap)
    check_member_was_used(eng, model, 1)
    eng.close()


def quad_host(c, k):
    """a quadratic likelihood in plain Python floats: the engine's host callback and the checker call the same function"""
    def f(x):
        acc = 0.0
        for d in range(len(c)):
            t = float(x[d]) - c[d]
            acc = acc + t * t * k[d]
        return acc
    return f


def user_like_pair(set_target_engine, host_fn, D=3, Nt=4, W=3):
    """a user likelihood (propose / accept passes) under the set {Gaussian, prior, Gaussian}: uniform, Gaussian and uniform prior
    dimensions, a `limit` bound inside the first one's support"""
    beta = E.geometric_ladder(Nt, 1e3)
    types, cen, hw = [E.PRIOR_UNIFORM, E.PRIOR_GAUSSIAN, E.PRIOR_UNIFORM], [0.2, -0.1, 0.4], [1.5, 0.8, 2.0]
    blo, bhi = [E.BOUND_LIMIT, E.BOUND_OPEN, E.BOUND_OPEN], [E.BOUND_LIMIT, E.BOUND_OPEN, E.BOUND_OPEN]
    bmin, bmax = [-1.2, 0.0, 0.0], [1.6, 0.0, 0.0]
    rng = np.random.default_rng(17)
    x0 = rng.uniform([-1.0, -0.8, -1.4], [1.4, 0.6, 2.2], size=(Nt * W, D))
    fac = np.tile([0.3, 0.2, 0.4], (Nt, 1)) / np.sqrt(beta)[:, None].clip(0.05)
    eng = E.Engine(D, Nt, W, swap_rate=0.3, seed=SEED)
    eng.set_bounds(blo, bhi, bmin, bmax)
    eng.set_prior(types, cen, hw)
    set_target_engine(eng)
    eng.set_ladder(beta)
    eng.set_proposals(E.PROP_DIAG, fac)
    eng.set_states(x0)
    pb = O.Problem(D)
    pb.set_bounds(blo, bhi, bmin, bmax)
    pb.set_prior(types, cen, hw)
    pb.set_user(host_fn)
    lad = O.Ladder(pb, beta, W=W, swap_rate=0.3)
    lad.set_proposals([(O.PROP_DIAG, fac[r], 0.0) for r in range(Nt)])
    lad.use_philox(SEED)
    lad.set_states(PU.to_oracle_order(x0, Nt, W))
    cum = cum_of([0.3, 0.4, 0.3])
    C_, S_, O_ = np.tile(cum, (Nt, 1)), np.tile([1.0, 1.0, 0.3], (Nt, 1)), np.tile([0.5, 0.0, 0.0], (Nt, 1))
    eng.set_proposal_mixture(C_, S_, O_)
    eng.set_proposal_prior_draw(1)
    chains = [PM.FixedSet(cum) for _ in range(Nt * W)]
    return eng, lad, PM.PriorDrawOracle(lad, SEED, chains, S_, O_, 1)


def device_like():
    """the torch device likelihood (torch is imported first, by the worker module this borrows the polynomial from)"""
    import device_like_worker as DW
    c, k = DW.poly_coefs(3)
    k = [v * 4.0 for v in k]
    eng, lad, model = user_like_pair(lambda e: e.set_target_device(DW.poly_torch(c, k)), DW.poly_numpy(c, k))
    assert eng.sweep_kernel_name.startswith("sweep_lanes_kernel<4, 1, true>"), eng.sweep_kernel_name
    assert eng.step_kernel_name.endswith(DW.SUFFIX), eng.step_kernel_name
    run(eng, lad, model, 40)
    check_member_was_used(eng, model, 1)
    eng.close()


if __name__ == "__main__":
    {"ragged_general": ragged_general, "device_like": device_like}[sys.argv[1]]()
    print("ok " + sys.argv[1])
