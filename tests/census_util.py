"""Runs one case of the census of kernel builds (tests/build_census.py): the engine of the case's configuration and its checker twin,
the reported kernel name against the table's, PT steps and plain sweeps with a full comparison after each round.  Shared by
tests/test_gpu_build_census.py (in its own process) and tests/census_worker.py (the cases under an environment switch)."""
import numpy as np

import aging_util as AU
import oracle_lib as O
import parity_util as PU
import proposal_pairs as PP
from ptmcmc_amd import engine as E

KIND = {"lower": E.PROP_LOWER, "dense": E.PROP_DENSE, "diag": E.PROP_DIAG}
CAP = 64          # history rows per chain: 13 PT steps save at most two rows each
SWAP_RATE = 0.3


def state_space(c):
    """the case's bounds, prior, target mean and start states, in units of the target's standard deviations: narrow limits on a few
    dimensions (the first ones and the last two, next to the padded lanes), so that a share of the proposals is invalid whatever the
    dimension; wrap and reflect boundaries and Gaussian prior factors for the general state space"""
    D, Nt, W = c["D"], c["Nt"], c["W"]
    pr = PU.problem_for(D, 2, 10.0)
    sig = np.sqrt(np.diag(pr.cov))
    rng = np.random.default_rng(D * 31 + Nt)
    bounds = prior = mean = x0 = None
    if c.get("bounds"):
        blo, bhi = [E.BOUND_OPEN] * D, [E.BOUND_OPEN] * D
        for d in {1 % D, 4 % D, D - 1}:
            blo[d] = E.BOUND_LIMIT
        for d in {2 % D, 4 % D, (D - 2) % D}:
            bhi[d] = E.BOUND_LIMIT
        if D > 128:     # (four chains only: one dimension in 64 limited on either side, so that their few proposals meet a limit -- with a
            #  quarter of them limited next to every proposal was invalid, and a case rested on one accepted move in 36, or on none)
            for d in range(D):
                if d % 64 == 1:
                    blo[d] = E.BOUND_LIMIT
                elif d % 64 == 2:
                    bhi[d] = E.BOUND_LIMIT
        if c["bounds"] == "wrap":
            blo[0] = bhi[0] = E.BOUND_WRAP
            dr = 3 if D > 3 else 1     # (three dimensions: the reflecting one takes the place of a limited one, not of the wrapped one)
            blo[dr] = bhi[dr] = E.BOUND_REFLECT
        # limits at 2 to 3 standard deviations up to 16 dimensions; beyond, a proposal moves a dimension by ~ 2.4 / sqrt(D) of them, and the
        # limits (and the start states inside them) shrink with it, so that the cold rungs meet them too
        near = min(1.0, 4.0 / np.sqrt(D))
        bounds = (blo, bhi, list(-rng.uniform(2.0, 3.0, D) * near * sig), list(rng.uniform(2.0, 3.0, D) * near * sig))
    if c.get("gauss_prior"):
        types, cen, hw = list(pr.types), list(pr.centers), list(pr.halfwidths)
        for d in {0, 2 % D, D - 1}:
            types[d], cen[d], hw[d] = E.PRIOR_GAUSSIAN, float(rng.normal() * 0.2 * sig[d]), float(rng.uniform(0.8, 2.0) * sig[d])
        prior = (types, cen, hw)
    if c.get("mean"):
        mean = rng.normal(size=D) * 0.3 * sig
    if bounds is not None or prior is not None:
        x0 = rng.uniform(-0.8, 0.8, size=(Nt * W, D)) * sig
        if bounds is not None:
            bounded = np.array([lo != E.BOUND_OPEN or hi != E.BOUND_OPEN for lo, hi in zip(bounds[0], bounds[1])])
            x0[:, bounded] *= near
            if D > 128:   # (the open dimensions start from draws of the target, widened as below and more: moves inwards gain; inside the prior's box)
                wide = 3.0 * rng.standard_normal((Nt * W, D)) @ np.linalg.cholesky(pr.cov).T
                wide = np.clip(wide, -0.75 * np.asarray(pr.halfwidths), 0.75 * np.asarray(pr.halfwidths))
                x0[:, ~bounded] = wide[:, ~bounded]
    elif D > 128:   # (beyond 128 dimensions a start drawn from the prior's box accepts next to nothing: start from draws of the target, widened)
        x0 = 1.5 * rng.standard_normal((Nt * W, D)) @ np.linalg.cholesky(pr.cov).T   # (over-dispersed: moves inwards gain)
    return dict(bounds=bounds, prior=prior, mean=mean, x0=x0, time_kernels=bool(c.get("time_kernels")))


class Case:
    """the engine and the checker (with the adaptive model where a set adapts) of one configuration"""

    def __init__(self, c, persistent=False):
        self.c = c
        self.persistent = persistent      # the persistent ladder kernel takes the PT steps: its statistics are part of every comparison
        D, Nt, W, kind = c["D"], c["Nt"], c["W"], KIND[c["kind"]]
        kw = self.space = state_space(c)
        self.model = None
        self.tracked = bool(c.get("hist")) or bool(c.get("de"))
        if c.get("ada"):
            top, scales, odfs = PP.one_level(3, 0.5)
            self.pr, self.eng, self.lad, self.model = PP.adaptive_pair(D, Nt, W, kind, top, scales, odfs, 0.3, cap=CAP if self.tracked else 0,
                                                                       evolve=c.get("evolve") or 0.0, swap_rate=SWAP_RATE, **kw)
        else:
            if c.get("de"):
                self.pr, self.eng, self.lad = PP.de_pair(D, Nt, W, kind, 1, 0.3, 10, c.get("mix") or 2, CAP, **kw)
            else:
                self.pr, self.eng, self.lad = PP.ladder_flavour_pair(D, Nt, W, kind, SWAP_RATE, c.get("oned") or 0.0, c.get("mix") or 0, c.get("hist") or 0,
                                                                     cap=CAP, tmax=1e2, **kw)
            if c.get("evolve"):
                self.eng.set_evolve_temps(c["evolve"]); self.lad.evolve_temps(c["evolve"])
        self.threads = 8 if Nt * W >= 1024 else 1

    def step(self, n):
        self.eng.step(n); self.eng.sync()
        self.model.step(n) if self.model else self.lad.pt_step(n, self.threads)

    def sweep(self, n):
        self.eng.sweep(n); self.eng.sync()
        self.model.sweep(n) if self.model else self.lad.sweep(n, self.threads)

    def compare(self, what):
        eng, lad, c = self.eng, self.lad, self.c
        if self.model:
            PP.assert_same_adaptive(eng, lad, self.model, what)
            if self.tracked:
                PP.assert_same_adaptive_history(eng, lad, self.model, CAP)
        else:
            PU.assert_same_state(eng, lad, what)
            if self.tracked:
                PU.assert_same_history_and_map(eng, lad, CAP)
        pairs, acc = eng.last_swaps()
        assert np.array_equal(pairs, lad.last_pairs) and np.array_equal(acc, lad.last_accept), what
        t, a = eng.swap_counts()
        assert np.array_equal(t, lad.swap_count) and np.array_equal(a, lad.swap_accept_count), what
        if c.get("evolve"):
            assert np.array_equal(eng.invtemps(), lad.betaw), "%s: temperatures differ" % what
        if self.persistent:
            st = eng.ladder_stats()
            assert st["launches"] > 0 and st["fallbacks"] == 0 and not st["disabled"], (what, st)

    def limits_changed_the_chains(self):
        """Did the narrow limits reject a proposal that would have been accepted?  A second checker ladder with the limits taken away
        (the same prior, mean, proposals, seed and start states) walks the case's steps: an open / limit boundary does nothing to a
        state but call it invalid, so chains that differ from the bounded checker's show that invalid proposals were met and mattered.
        (Fixed Gaussian sets only: the cases with limits that draw differential evolution or adapt have siblings here that do not.)"""
        c, lad, kw = self.c, self.lad, self.space
        pb = PU.oracle_problem(self.pr, None, kw["prior"], kw["mean"])
        twin = O.Ladder(pb, self.pr.beta, W=lad.W, swap_rate=SWAP_RATE, add_every_N=max(c.get("hist") or 0, 1))
        twin.set_proposals(lad._prop_specs)
        for r in range(lad.Nt):
            twin._props[r].K, twin._props[r].mix = lad._props[r].K, lad._props[r].mix
        twin.use_philox(PP.SEED)
        twin.set_states(PU.to_oracle_order(kw["x0"], lad.Nt, lad.W))
        if c.get("evolve"):
            twin.evolve_temps(c["evolve"])
        for _ in range(3):
            twin.pt_step(3, self.threads)
        twin.sweep(2, self.threads); twin.pt_step(2, self.threads)
        return not np.array_equal(twin.x, lad.x)

    def close(self):
        self.eng.close()


def assert_reported_name(eng, name):
    """the build the engine reports: string for string the table's name"""
    if name.startswith("sweep_"):
        assert eng.sweep_kernel_name == name, (eng.sweep_kernel_name, name)
        assert eng.step_kernel_name == "decide_kernel + " + name, (eng.step_kernel_name, name)
    else:
        assert eng.step_kernel_name == name, (eng.step_kernel_name, name)


def run_case(name, c):
    """the whole case; returns what it saw (for the worker's line).  Every assertion is the test's."""
    case = Case(c, persistent=name.startswith("ladder_persistent_kernel<"))
    eng = case.eng
    try:
        assert_reported_name(eng, name)
        done = 0
        for _ in range(3):
            case.step(3); done += 3
            case.compare("after %d PT steps" % done)
        case.sweep(2)
        case.compare("after 2 plain sweeps")
        case.step(2)
        case.compare("after 2 more PT steps")
        # the case can fail for a real reason: moves were accepted and rejected, exchanges were tried, the moves the build is for were made
        tries, acc = int(eng.ntries.sum() - eng.Nc), int(eng.naccept.sum() - eng.Nc)
        assert 0 < acc < tries, (acc, tries)
        assert int(eng.swap_counts()[0].sum()) > 0
        lt = set(int(v) for v in np.unique(eng.last_type)) - {-1}
        if c.get("de"):
            assert lt & {0, 10}, lt                       # differential evolution is member 0: parallel moves 0, snooker moves 10
        if c.get("oned") and not c.get("ada"):
            assert (any(v // 10 == 1 for v in lt) if c.get("mix") else 1 in lt), lt
        # (asked of the populations of 15 chains and more: the four chains beyond 128 dimensions make 36 proposals in all, of which a
        #  handful is accepted -- too few for one of them to be both invalid and acceptable without its limit)
        if c.get("bounds") == "limit" and not (c.get("de") or c.get("ada")) and c["D"] <= 128:
            assert case.limits_changed_the_chains(), "no proposal that the open twin accepted was invalid: the limits are too wide to bite"
        if c.get("evolve") and int(eng.swap_counts()[1].sum()) > 0:       # (an accepted exchange pries its gap open)
            assert not np.array_equal(eng.invtemps(), np.tile(case.pr.beta, (eng.W, 1)))
        return dict(name=name, accepted=acc, tries=tries, swaps=int(eng.swap_counts()[1].sum()))
    finally:
        case.close()


AGED_ROUNDS = 7      # PT steps and plain sweeps of a case after it was aged: step(3), sweep(2), step(2)


def run_case_aged(name, c):
    """the same case late in a run (tests/aging_util.py): one young round, then engine and checker are put at PT step 2^32 - 2 with every
    chain's counters shifted as close to PTM_COUNT_MAX as leaves the rounds 16 below it -- differential evolution keeps its Nhist, its
    ring may not wrap -- and step(3), sweep(2), step(2) follow, each with the full comparison.  The first of them takes the steps
    2^32 - 2 .. 2^32 in ONE call: the step kernels cross the word boundary of the step number inside a launch."""
    case = Case(c, persistent=name.startswith("ladder_persistent_kernel<"))
    eng = case.eng
    try:
        assert_reported_name(eng, name)
        case.step(3)
        case.compare("young, after 3 PT steps")
        case.eng, d = AU.age_pair(eng, case.lad, AGED_ROUNDS, shift_nhist=not c.get("de"), adaptive=bool(c.get("ada")))
        assert_reported_name(eng, name)
        assert eng.step_count == case.lad.step == AU.LATE_STEP
        case.compare("aged by %d" % d)

        def sums():
            t, a = eng.counter_sums()
            nt, na = eng.ntries.astype(np.int64), eng.naccept.astype(np.int64)
            assert (t, a) == (int(nt.sum()), int(na.sum())), ((t, a), int(nt.sum()), int(na.sum()))
            assert (na <= nt).all() and nt.min() >= d
            return t, a
        t0, a0 = sums()
        assert d > 2**30 and t0 > 2**32      # (four chains at the least: the sums are past 32 bits)
        case.step(3)
        assert eng.step_count == case.lad.step == 2**32 + 1
        case.compare("aged, after the 3 PT steps across 2^32")
        case.sweep(2)
        case.compare("aged, after 2 plain sweeps")
        case.step(2)
        assert eng.step_count == case.lad.step == 2**32 + 5
        case.compare("aged, after 2 more PT steps")
        t1, a1 = sums()
        tries, acc = t1 - t0, a1 - a0
        assert 0 < acc < tries, (acc, tries)
        top = max(int(eng.ntries.max()), int(eng.nhist.max()))
        assert top <= AU.COUNT_MAX - AU.MARGIN, top
        assert top > AU.COUNT_MAX - AU.MARGIN - AU.ADDS_PER_STEP * AGED_ROUNDS - max(c.get("hist") or 1, 1) * CAP - 16, top     # (and it did run late)
        return dict(name=name, accepted=acc, tries=tries, swaps=int(eng.swap_counts()[1].sum()), top=top)
    finally:
        case.eng = eng
        case.close()
