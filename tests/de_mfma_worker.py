"""One case of differential evolution on the matrix cores (de_mfma32_kernel) against the CPU oracle, in a process of its own: the engine
reads PTM_DE_MFMA and PTM_LADDER once per process (tests/test_gpu_de_mfma.py sets PTM_DE_MFMA=1 PTM_LADDER=0).  Engine and oracle are
built by proposal_pairs.de_pair; states, scalars, counters, every saved row and the MAPs are compared bit for bit.
usage: python de_mfma_worker.py CASE [aged]     prints "ok key=value ..."
(aged: after the case's first PT step engine and oracle are put late in a run, tests/aging_util.py -- PT step 2^32 - 2, Ntries and Naccept
shifted up to 16 below PTM_COUNT_MAX at the run's end; Nhist stays, differential evolution's ring may not wrap)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ptmcmc_amd import engine as E
import parity_util as PU
from proposal_pairs import de_pair

# D, Nt, W, kind, add_every_N, snooker, n_init_extra (in units of D), K Gaussians, steps
CASES = {
    "one_wave": (32, 3, 64, E.PROP_DENSE, 1, 0.3, 10, 2, 30),        # one wave per rung, no pad lane
    "straddle": (21, 4, 320, E.PROP_LOWER, 2, 0.2, 10, 6, 30),       # pad dimensions, tiles that straddle rungs, every second add saved, six Gaussians
    "snooker_diag": (17, 2, 128, E.PROP_DIAG, 1, 1.0, 40, 1, 30),    # snooker only, a diagonal factor as a Cholesky factor
    "parallel": (20, 3, 64, E.PROP_LOWER, 1, 0.0, 12, 2, 30),        # parallel moves only
    "no_init": (17, 2, 64, E.PROP_LOWER, 1, 0.3, 0, 2, 200),         # no initial rows: passed over until 10 D = 170 rows are saved
    "evolving": (32, 6, 64, E.PROP_DENSE, 1, 0.3, 12, 2, 40),        # evolving ladders
    "limit_mean": (24, 3, 64, E.PROP_LOWER, 1, 0.3, 10, 3, 30),      # limit bounds on a few dimensions, a target mean
}


def limit_mean_kw(D, Nt, W):
    """`limit` bounds on four dimensions (one of them one-sided), tight enough for the hot rungs to run into them, and a mean"""
    pr = PU.problem_for(D, Nt, 1e3)
    c, h = np.asarray(pr.centers, float), np.asarray(pr.halfwidths, float)
    blo, bhi = [E.BOUND_OPEN] * D, [E.BOUND_OPEN] * D
    for d in (1, 5, 20):
        blo[d] = bhi[d] = E.BOUND_LIMIT
    bhi[9] = E.BOUND_LIMIT
    rng = np.random.default_rng(77)
    x0 = c + 0.04 * h * rng.uniform(-1.0, 1.0, size=(Nt * W, D))
    return dict(bounds=(blo, bhi, list(c - 0.05 * h), list(c + 0.05 * h)), mean=c + 0.002 * h * rng.normal(size=D), x0=x0)


def kind_name(kind, ev):
    return "de_mfma32_kernel<%d, %s>" % (0 if kind == E.PROP_DENSE else 2, "true" if ev else "false")


def types_in(he, nsize, first, last):
    """the types of the accepted moves the saved rows first .. last - 1 hold (rows every chain has)"""
    return set(int(v) for s_ in range(first, min(last, int(nsize.min()))) for v in np.unique(he["last_type"][s_]))


def check_types(seen, snooker, K):
    if snooker < 1.0:
        assert 0 in seen, seen
    if snooker > 0.0:
        assert 10 in seen, seen
    assert any(1 <= (v % 10) <= K for v in seen), seen


def run_steps(case, aged=False):
    D, Nt, W, kind, N, snooker, ninit, K, steps = CASES[case]
    cap = 2 * steps + 8
    ev = case == "evolving"
    kw = limit_mean_kw(D, Nt, W) if case == "limit_mean" else {}
    pr, eng, lad = de_pair(D, Nt, W, kind, N, snooker, ninit, K, cap, **kw)
    if ev:
        eng.set_evolve_temps(0.01); lad.evolve_temps(0.01)
    assert eng.sweep_kernel_name == kind_name(kind, ev), eng.sweep_kernel_name
    assert eng.step_kernel_name == "decide_kernel + " + kind_name(kind, ev), eng.step_kernel_name
    done = 0
    for n in (1, 4, steps - 5):
        eng.step(n); eng.sync(); lad.pt_step(n)
        done += n
        PU.assert_same_state(eng, lad, "after %d PT steps" % done)
        if ev:
            assert np.array_equal(eng.invtemps(), lad.betaw), done
        if aged and done == 1:
            import aging_util as AU
            AU.age_pair(eng, lad, steps - 1, shift_nhist=False)
            assert eng.step_count == lad.step == AU.LATE_STEP and eng.sweep_kernel_name == kind_name(kind, ev)
            PU.assert_same_state(eng, lad, "aged")
            ck0 = eng.naccept.astype(np.int64)
    if aged:
        top = int(eng.ntries.max())
        assert eng.step_count == lad.step == AU.LATE_STEP + steps - 1
        assert AU.COUNT_MAX - AU.MARGIN - 2 * steps <= top <= AU.COUNT_MAX - AU.MARGIN, top
    PU.assert_same_history_and_map(eng, lad, cap)
    he, nsize = eng.history(), eng.nsize
    if case == "no_init":
        # row s was saved by add s: the member is ready from 10 D rows on, so the adds that saw fewer than that drew Gaussians alone
        ready = 10 * D
        early, late = types_in(he, nsize, 0, ready), types_in(he, nsize, ready + 1, 1 << 30)
        assert not [v for v in early if v % 10 == 0], early
        check_types(late, snooker, K)
    else:
        check_types(types_in(he, nsize, 0, 1 << 30), snooker, K)
    if case == "limit_mean":
        tries, acc = eng.ntries.sum() - eng.Nc, eng.naccept.sum() - eng.Nc
        assert 0 < acc < tries
    out = "kernel=%s accepts=%d" % (eng.sweep_kernel_name.replace(" ", ""), int((eng.naccept.astype(np.int64) - ck0).sum()) if aged else int(eng.naccept.sum() - eng.Nc))
    eng.close()
    return out


def run_late():
    """differential evolution late in a run (tests/aging_util.py: late_de_pair): 128 saved rows at a history stride of 2^24, Nhist = 127 * 2^24 - 2,
    PT step 2^32 - 2; five initial rows per dimension make the member ready at 21 dimensions"""
    import aging_util as AU
    D, Nt, W, kind = 21, 4, 128, E.PROP_LOWER
    pr, eng, lad = AU.late_de_pair(D, Nt, W, kind, snooker=0.3, ninit=5, K=3)
    assert eng.step_kernel_name == "decide_kernel + " + kind_name(kind, False), eng.step_kernel_name
    seen = AU.run_late_de(eng, lad)
    out = "kernel=%s types=%s" % (eng.sweep_kernel_name.replace(" ", ""), ",".join(str(v) for v in sorted(seen)))
    eng.close()
    return out


def run_sweeps():
    """plain sweeps, and sweeps over two rung ranges (the second closes the step), against the oracle's plain sweeps"""
    D, Nt, W, kind, N, snooker, ninit, K, steps = CASES["straddle"]
    cap = 64
    pr, eng, lad = de_pair(D, Nt, W, kind, N, snooker, ninit, K, cap)
    assert eng.sweep_kernel_name == kind_name(kind, False), eng.sweep_kernel_name
    eng.step(3); eng.sync(); lad.pt_step(3)
    PU.assert_same_state(eng, lad, "after 3 PT steps")
    eng.sweep(4); eng.sync(); lad.sweep(4)
    PU.assert_same_state(eng, lad, "after 4 plain sweeps")
    for k in range(5):
        eng.sweep_rungs(0, 1, False); eng.sweep_rungs(1, Nt - 1, True)
    eng.sync(); lad.sweep(5)
    PU.assert_same_state(eng, lad, "after 5 sweeps over two rung ranges each")
    eng.step(2); eng.sync(); lad.pt_step(2)
    PU.assert_same_state(eng, lad, "after 2 more PT steps")
    PU.assert_same_history_and_map(eng, lad, cap)
    eng.close()
    return "kernel=" + kind_name(kind, False).replace(" ", "")


def run_short_ring():
    """a ring that loses rows the draw asks for: the error of the general kernel's draw, from this kernel"""
    pr, eng, lad = de_pair(32, 2, 64, E.PROP_DENSE, 1, 0.1, 10, 2, cap=16)
    assert eng.sweep_kernel_name == kind_name(E.PROP_DENSE, False), eng.sweep_kernel_name
    eng.step(80)
    try:
        eng.sync()
    except E.PtmError as ex:
        assert "history" in str(ex), str(ex)
        eng.close()
        return "error=history"
    raise AssertionError("a ring too short for the run went unreported")


def name_gen2():
    """wrap bounds and a Gaussian prior: not the box-bounds build's state space"""
    D, Nt, W = 24, 3, 64
    pr = PU.problem_for(D, Nt, 1e3)
    c, h = np.asarray(pr.centers, float), np.asarray(pr.halfwidths, float)
    blo, bhi = [E.BOUND_OPEN] * D, [E.BOUND_OPEN] * D
    blo[3] = bhi[3] = E.BOUND_WRAP
    types = [E.PRIOR_UNIFORM] * D
    types[5] = E.PRIOR_GAUSSIAN
    pr, eng, lad = de_pair(D, Nt, W, E.PROP_LOWER, 1, 0.3, 10, 2, 64, bounds=(blo, bhi, list(c - h), list(c + h)), prior=(types, list(c), list(h)))
    names = [eng.sweep_kernel_name]
    eng.close()
    for what in ("wrap", "gauss"):   # ... and each of the two alone
        kw = dict(bounds=(blo, bhi, list(c - h), list(c + h))) if what == "wrap" else dict(prior=(types, list(c), list(h)))
        pr, eng, lad = de_pair(D, Nt, W, E.PROP_LOWER, 1, 0.3, 10, 2, 64, **kw)
        names.append(eng.sweep_kernel_name)
        eng.close()
    return "kernel=" + "|".join(n.replace(" ", "") for n in names)


def name_prior_draw():
    pr, eng, lad = de_pair(24, 3, 64, E.PROP_LOWER, 1, 0.3, 10, 2, 64)
    assert eng.sweep_kernel_name == kind_name(E.PROP_LOWER, False), eng.sweep_kernel_name
    eng.set_proposal_prior_draw(1)
    name = eng.sweep_kernel_name
    eng.close()
    return "kernel=" + name.replace(" ", "")


if __name__ == "__main__":
    case = sys.argv[1]
    if case in CASES:
        res = run_steps(case, aged=sys.argv[2:] == ["aged"])
    elif case == "late":
        res = run_late()
    elif case == "sweeps":
        res = run_sweeps()
    elif case == "short_ring":
        res = run_short_ring()
    elif case == "name_gen2":
        res = name_gen2()
    elif case == "name_prior_draw":
        res = name_prior_draw()
    else:
        raise SystemExit("unknown case " + case)
    print("ok " + res)
