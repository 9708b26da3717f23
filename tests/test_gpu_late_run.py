"""Every kernel late in a run: PT steps past 2^32, chain counters near PTM_COUNT_MAX = 2^31 - 1 (tests/aging_util.py puts an engine and
its checker twin there; tests/test_late_run_cpu.py shows that the ageing itself changes no chain and that a 32-bit step anywhere would
part the chains at once).

  - the whole census of kernel builds (tests/build_census.py), aged: census_util.run_case_aged;
  - the horizon itself (include/ptm_engine.h, PTM_COUNT_MAX): the step that fits is taken and equals the checker, the call that could pass
    the limit is refused with nothing changed, ptm_restore refuses counters outside it;
  - the estimators on an aged ring;
  - the paths the census does not hold, one small aged case each, through the existing builders and workers;
  - differential evolution at Nhist ~ 2.1e9 in every kernel that draws it (aging_util.late_de_pair);
  - ptm_restore under a two-sided reflection, which the aged census found enforcing saved states a second time.

No test steps a kernel past PTM_COUNT_MAX; the refusals launch nothing; every aged parity run ends at least 16 below the limit (the three
engines of the limit test, which the guard itself keeps at or below it, excepted)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aging_util as AU
import build_census as BC
import census_util as CU
import history_readers_util as HU
import parity_util as PU
import proposal_pairs as PP
from ptmcmc_amd import engine as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_children = {}


def child_lines(switch):
    """(status, lines by case name, the end of stderr) of the switch's child process (tests/census_worker.py SWITCH aged), started once"""
    if switch not in _children:
        var, value = switch.split("=")
        env = dict(os.environ)
        env[var] = value
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "census_worker.py"), switch, "aged"], env=env, capture_output=True, text=True, timeout=300)
            status, out, err = "exit status %d" % r.returncode, r.stdout, r.stderr
        except subprocess.TimeoutExpired as e:
            text = lambda b: b.decode(errors="replace") if isinstance(b, bytes) else (b or "")
            status, out, err = "timed out after 300 s", text(e.stdout), text(e.stderr)
        except Exception as e:
            status, out, err = "not started: %r" % (e,), "", ""
        lines = {}
        for ln in out.splitlines():
            if ln.startswith("{"):
                try:
                    d = json.loads(ln)
                except ValueError:
                    continue
                lines[d["name"]] = d
        _children[switch] = (status, lines, err[-2000:])
    return _children[switch]


@pytest.mark.parametrize("name", sorted(BC.CASES))
def test_the_build_computes_the_checkers_chains_late_in_a_run(name):
    """census_util.run_case_aged: one young round, the ageing, step(3) across 2^32, sweep(2), step(2), each compared in full; the counter
    sums against int64 numpy sums, the step count, and `0 < accepted < tries` over the aged rounds.  (The four-chain cases beyond 128
    dimensions with limits make 23 proposals there; census_util.state_space limits one dimension in 64 of theirs and starts the open ones
    over-dispersed, so that the thinnest of them, the diagonal factor at 509 dimensions, still has a move accepted.)"""
    c = BC.CASES[name]
    if c.get("env"):
        status, lines, err = child_lines(c["env"])
        assert name in lines, "the child process of %s (%s) printed no line for this case\n%s" % (c["env"], status, err)
        assert lines[name]["ok"], lines[name]["error"]
        seen = lines[name]
    else:
        seen = CU.run_case_aged(name, c)
    assert 0 < seen["accepted"] < seen["tries"]
    assert seen["top"] <= AU.COUNT_MAX - AU.MARGIN


# ---- the limit itself -------------------------------------------------------------------------------------------------------------
LIMIT_CAP = 112      # 16 * 7 divides 2^31 - 16 = 16 * 7 * 73 * 262657: counters that stand at 10 are shifted to PTM_COUNT_MAX - 5 by a whole number of ring periods
YOUNG_TOP = 10
LIMIT_ENGINES = {
    # name: (D, Nt, W, kind, one-dimensional fraction, history, the kernel of its PT steps)
    "matrix cores with history": (21, 5, 64, E.PROP_LOWER, 0.0, True, r"decide_kernel \+ sweep_mfma32_kernel<2, true, 0, false, false>"),
    "persistent ladder kernel with history": (5, 5, 3, E.PROP_LOWER, 0.0, True, r"ladder_persistent_kernel<8, 0, 2>"),
    "general kernel": (5, 5, 64, E.PROP_DENSE, 0.4, False, r"decide_kernel \+ sweep_kernel<8, 0, true, false>"),
}


def _snapshot(eng):
    s = dict(x=eng.states(), step=eng.step_count, swaps=eng.swap_counts())
    for name in ("llike", "lprior", "ntries", "naccept", "nhist", "last_type"):
        s[name] = getattr(eng, name)
    if eng.hist_rungs:
        s["history"] = eng.history()
        s["map"] = eng.map()
    return s


def _assert_unchanged(eng, before, what):
    now = _snapshot(eng)
    assert now["step"] == before["step"], what
    for name in ("x", "llike", "lprior", "ntries", "naccept", "nhist", "last_type"):
        assert np.array_equal(now[name], before[name]), (what, name)
    assert all(np.array_equal(a, b) for a, b in zip(now["swaps"], before["swaps"])), what
    for part in ("history", "map"):
        if part in before:
            for k in before[part]:
                assert np.array_equal(now[part][k], before[part][k], equal_nan=now[part][k].dtype.kind == "f"), (what, part, k)


@pytest.mark.parametrize("which", sorted(LIMIT_ENGINES))
def test_the_horizon_is_enforced_and_the_last_steps_before_it_are_the_checkers(which):
    D, Nt, W, kind, odf, hist, kernel = LIMIT_ENGINES[which]
    import re
    pr, eng, lad = PP.ladder_flavour_pair(D, Nt, W, kind, 0.3, odf, 0, 1 if hist else 0, cap=LIMIT_CAP, tmax=1e2, time_kernels=not which.startswith("persistent"))
    view = eng

    def compare(what):
        PU.assert_same_state(view, lad, what)
        if hist:
            PU.assert_same_history_and_map(view, lad, LIMIT_CAP)
        assert view.step_count == lad.step, what

    try:
        assert re.fullmatch(kernel, eng.step_kernel_name), eng.step_kernel_name
        eng.step(3); eng.sync(); lad.pt_step(3)
        n = YOUNG_TOP - int(max(eng.nhist.max(), eng.ntries.max()))
        assert 0 <= n <= YOUNG_TOP - 3        # plain sweeps add exactly one to every chain: the largest counter comes to stand at YOUNG_TOP
        eng.sweep(n); eng.sync(); lad.sweep(n)
        compare("young")
        d = AU.COUNT_MAX - 5 - YOUNG_TOP
        assert d % LIMIT_CAP == 0
        view = AU.AgedView(eng, AU.age_engine(eng, AU.LATE_STEP, d, 1))
        AU.age_checker(lad, AU.LATE_STEP, d)
        assert int(max(eng.nhist.max(), eng.ntries.max())) == AU.COUNT_MAX - 5
        compare("at the limit - 5")
        # two steps fit: (limit - 5) + 2 * 2 <= limit
        eng.step(2); eng.sync(); lad.pt_step(2)
        compare("after the 2 steps that fit")
        top = int(max(eng.nhist.max(), eng.ntries.max()))
        assert AU.COUNT_MAX - 3 <= top <= AU.COUNT_MAX - 1
        # ten more do not: refused, nothing queued, nothing changed, the message names the limit and the remedy
        before = _snapshot(eng)
        for call in (eng.step, eng.sweep):
            with pytest.raises(E.PtmError) as err:
                call(10)
            msg = str(err.value)
            assert msg.startswith("ptm error -2:") and str(AU.COUNT_MAX) in msg and "PTM_COUNT_MAX" in msg and "INTEGRATION.md" in msg, msg
            eng.sync()
            _assert_unchanged(eng, before, "after the refused call")
        compare("after the refusals")
        # the engine stays usable: one step, if it fits the rule (a chain in two exchange trials in both steps stands at limit - 1)
        if top + 2 <= AU.COUNT_MAX:
            eng.step(1); eng.sync(); lad.pt_step(1)
            compare("after one more step")
            assert int(max(eng.nhist.max(), eng.ntries.max())) <= AU.COUNT_MAX
        else:
            with pytest.raises(E.PtmError):
                eng.step(1)
        assert top + 2 <= AU.COUNT_MAX, "the case was meant to have room for one more step (top = %d)" % top
        # ptm_restore: counters outside [0, PTM_COUNT_MAX] and naccept > ntries are refused, and the engine is as before
        before = _snapshot(eng)
        ck = eng.checkpoint()
        for field, value in (("nhist", AU.COUNT_MAX + 1), ("nhist", 2**32 - 1), ("nhist", -1), ("ntries", -1), ("naccept", None)):
            bad = dict(ck)
            bad[field] = ck[field].copy()
            bad[field][-1] = ck["ntries"][-1] + 1 if value is None else value
            if field == "ntries":
                bad["naccept"] = ck["naccept"].copy(); bad["naccept"][-1] = -1     # (so that the negative count itself is what is wrong)
            with pytest.raises(E.PtmError) as err:
                eng.restore(bad)
            assert str(err.value).startswith("ptm error -1:") and field in str(err.value), str(err.value)
            _assert_unchanged(eng, before, "after the refused restore of %s" % field)
        compare("after the refused restores")
    finally:
        eng.close()


# ---- the estimators on an aged ring -----------------------------------------------------------------------------------------------
AGED_RING = dict(D=2, Nt=6, W=70, add=3, steps=300, ilen=200, cap=75, evolve=0.01, seed=0xE71D7, swap_rate=0.4)
ESTIMATOR_MAX = 2000000000     # ptm_log_evidence and ptm_ess_* refuse beyond: "more than 2e9 steps"


def test_log_evidence_on_an_aged_ring_and_the_estimators_refusal_beyond_2e9_adds():
    r = AGED_RING
    make = lambda: HU.make_engine(r["D"], r["Nt"], r["W"], "lower", r["add"], r["seed"], r["swap_rate"], r["Nt"], r["cap"], r["evolve"])
    young, aged = make(), make()
    try:
        for e in (young, aged):
            e.step(r["steps"]); e.sync()
        assert np.array_equal(young.states(), aged.states())
        unit = r["add"] * r["cap"]
        d = (ESTIMATOR_MAX - AU.MARGIN - int(aged.nhist.max())) // unit * unit
        AU.age_engine(aged, young.step_count, d, r["add"])      # (the step stays: the twins go on together below)
        nh = aged.nhist
        assert ESTIMATOR_MAX - AU.MARGIN - unit < nh.max() <= ESTIMATOR_MAX - AU.MARGIN and len(set(nh.tolist())) > 1
        h = aged.history()
        assert h["row"].max() == 1 + (nh.max() - 1) // r["add"] and h["row"].max() >= r["cap"]      # a wrapped ring of late rows
        got = aged.log_evidence(r["ilen"])
        HU.assert_evidence(got, HU.evidence_model(h, nh, aged.invtemps(), r["Nt"], r["W"], r["ilen"], r["add"]), "against the model")
        # the window depends on nhist only through the shift: the young twin's answer, bit for bit
        HU.assert_evidence(got, young.log_evidence(r["ilen"]), "against the young twin")
        assert np.isfinite(got[0]).all() and got[3].min() > 0
        # past 2e9 adds both estimators refuse, and leave their outputs alone
        d2 = (AU.COUNT_MAX - AU.MARGIN - int(aged.nhist.max())) // unit * unit
        AU.age_engine(aged, young.step_count, d2, r["add"])
        assert ESTIMATOR_MAX < aged.nhist.max() <= AU.COUNT_MAX - AU.MARGIN
        with pytest.raises(E.PtmError) as err:
            aged.ess_windowed(1, None, 90, 3, 2)
        assert str(err.value).startswith("ptm error -2:") and "more than 2e9 steps" in str(err.value)
        with pytest.raises(E.PtmError) as err:
            aged.effective_samples(1, None, 90, 3)
        assert str(err.value).startswith("ptm error -2:") and "more than 2e9 steps" in str(err.value)
        out = (np.full(r["W"], 7.0), np.full((r["Nt"] - 1, r["W"]), 7.0), np.full((r["Nt"] - 1, r["W"]), 7.0), np.full((r["Nt"], r["W"]), 7, dtype=np.int32))
        with pytest.raises(E.PtmError) as err:
            aged.log_evidence(r["ilen"], out=out)
        assert str(err.value).startswith("ptm error -2:") and "more than 2e9 steps" in str(err.value)
        assert all((o == 7).all() for o in out)
        # and the chains go on all the same: the aged engine and the young twin take the same steps
        young.step(5); aged.step(5); young.sync(); aged.sync()
        assert np.array_equal(young.states(), aged.states()) and np.array_equal(young.nhist + d + d2, aged.nhist)
        assert aged.step_count == young.step_count == r["steps"] + 5
    finally:
        young.close(); aged.close()


# ---- paths the census does not hold -----------------------------------------------------------------------------------------------
def late_rounds(eng, lad, advance, compare, shift_nhist=True, adaptive=False):
    """one young round, the ageing (tests/aging_util.py), then step(3) -- across 2^32 in one call --, sweep(2), step(2), compared after
    each.  advance(n, sweep) moves engine and checker alike, compare(engine or its aged view, what) holds them together."""
    advance(3, False)
    compare(eng, "young, after 3 PT steps")
    view, d = AU.age_pair(eng, lad, CU.AGED_ROUNDS, shift_nhist=shift_nhist, adaptive=adaptive)
    assert eng.step_count == lad.step == AU.LATE_STEP
    compare(view, "aged by %d" % d)
    advance(3, False)
    assert eng.step_count == lad.step == 2**32 + 1
    compare(view, "aged, after the 3 PT steps across 2^32")
    advance(2, True)
    compare(view, "aged, after 2 plain sweeps")
    advance(2, False)
    compare(view, "aged, after 2 more PT steps")
    top = int(max(eng.ntries.max(), eng.nhist.max()))
    assert 2**31 - 2**16 < top <= AU.COUNT_MAX - AU.MARGIN, top
    return view, d


def plain_advance(eng, lad):
    def advance(n, sweep):
        (eng.sweep if sweep else eng.step)(n); eng.sync()
        (lad.sweep if sweep else lad.pt_step)(n)
    return advance


def _worker(script, args, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, script)] + list(args), env=e, capture_output=True, text=True, timeout=300)   # (a worker takes seconds: the limit only ends a hung one)
    if r.returncode < 0 or r.returncode in (134, 139):   # a crashed child (abort, fault): start nothing more on the device
        pytest.exit("%s %s died (exit %d)\n%s" % (script, args, r.returncode, r.stderr[-6000:]), returncode=1)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-6000:])
    return r.stdout


def test_box_prepass_and_row_labels_late_in_a_run():
    """12 rungs x 1024 walkers at 32 dimensions: label-swapping exchange phases, the forced box pre-pass on a grid of two blocks, the
    compacted sweep whose one add per chain the engine counts itself -- the worker's run against the checker, aged after its first leg"""
    out = _worker("box_prefilter_worker.py", ["aged"], {"PTM_BOX_PREFILTER": "1", "PTM_PREFILTER_GRID": "2"})
    assert out.startswith("ok "), out
    c = {k: int(v) for k, v in (kv.split("=") for kv in out.split()[1:])}
    assert c["eligible"] == 1 and c["rungs_flagged"] == c["rungs"] == 12 and 0 < c["settled"] < c["seen"] and c["accepts"] > 0, c


def test_differential_evolution_on_the_matrix_cores_late_in_a_run():
    out = _worker("de_mfma_worker.py", ["straddle", "aged"], {"PTM_DE_MFMA": "1", "PTM_LADDER": "0"})
    assert out.startswith("ok ") and "kernel=de_mfma32_kernel<2,false>" in out and int(out.split("accepts=")[1].split()[0]) > 0, out


def test_device_likelihood_late_in_a_run():
    out = _worker("device_like_worker.py", ["lanes", json.dumps([12, 6, 3, 0.0, True])], {})
    assert "OK lanes" in out, out


@pytest.mark.parametrize("D,W,kernel", [(12, 3, "sweep_lanes_kernel<16"), (5, 64, "sweep_kernel<8")])
def test_host_callback_likelihood_late_in_a_run(D, W, kernel):
    """the propose and accept passes around a host call (the shape of test_host_callback_likelihood_through_the_lanes_kernel; whole
    waves per rung at 5 dimensions: the general kernel's passes)"""
    import math
    import oracle_lib as O
    Nt = 8
    rng = np.random.default_rng(7)
    sc = rng.uniform(0.5, 2.0, D)
    loglike = lambda x: float(-0.5 * np.sum((np.asarray(x, dtype=np.float64) * sc) ** 2) - 0.1 * math.cos(3.0 * x[0]))
    beta = E.geometric_ladder(Nt, 1e3)
    blo, bhi, bmin, bmax = [0] * D, [0] * D, [0.0] * D, [0.0] * D
    blo[1], bhi[1], bmin[1], bmax[1] = 3, 3, -2.0, 2.0                     # wrap
    types, cen, hw = [1] * D, [0.0] * D, [4.0] * D
    types[2], cen[2], hw[2] = 2, 0.2, 1.5                                   # gaussian
    x0 = rng.uniform(-1.5, 1.5, size=(Nt * W, D))
    fac = np.tile(np.full(D, 0.4), (Nt, 1)) / np.sqrt(beta)[:, None].clip(1e-2)
    eng = E.Engine(D, Nt, W, swap_rate=0.3)
    try:
        eng.set_bounds(blo, bhi, bmin, bmax); eng.set_prior(types, cen, hw); eng.set_target_callback(loglike); eng.set_ladder(beta)
        eng.set_proposals(E.PROP_DIAG, fac, np.full(Nt, 0.3))
        eng.set_states(x0)
        assert eng.sweep_kernel_name.startswith(kernel), eng.sweep_kernel_name
        pb = O.Problem(D)
        pb.set_bounds(blo, bhi, bmin, bmax); pb.set_prior(types, cen, hw); pb.set_user(loglike)
        lad = O.Ladder(pb, beta, W=W, swap_rate=0.3)
        lad.set_proposals([(O.PROP_DIAG, fac[r], 0.3) for r in range(Nt)])
        lad.use_philox(0x5EED0001)
        lad.set_states(PU.to_oracle_order(x0, Nt, W))
        view, d = late_rounds(eng, lad, plain_advance(eng, lad), lambda e, what: PU.assert_same_state(e, lad, what))
        assert int(eng.naccept.astype(np.int64).sum()) - eng.Nc * (1 + d) > 5
    finally:
        eng.close()


def test_host_proposals_are_handed_the_late_step():
    """ptm_set_proposal_callback: the callback's `step` argument is the 64-bit PT step -- 2^32 + k once the run is there -- and the scripted
    proposal, a function of it, gives engine and checker the same chains (general state space, history of every second add)"""
    import oracle_lib as O
    from ptmcmc_amd.problems import GaussianProblem
    from test_gpu_host_proposals import scripted_proposal
    D, Nt, W, N, sr, cap, seed = 6, 8, 4, 2, 0.35, 96, 0x5EED0001
    pr = GaussianProblem(D, Nt, 1e3)
    blo, bhi, bmin, bmax = [0] * D, [0] * D, [0.0] * D, [0.0] * D
    blo[0], bhi[0], bmin[0], bmax[0] = 3, 3, -3.0, 2.5
    blo[2], bhi[2], bmin[2], bmax[2] = 1, 1, -6.0, 6.0
    bounds = (blo, bhi, bmin, bmax)
    types, cen, hw = [1] * D, [0.0] * D, [8.0] * D
    types[1], cen[1], hw[1] = 2, 0.1, 2.0
    prior, mean = (types, cen, hw), np.linspace(-0.3, 0.3, D)
    scale = 2.0 / np.sqrt(D) / np.sqrt(np.maximum(pr.beta, 0.02)) * np.sqrt(np.diag(pr.cov).mean())
    inner, seen = scripted_proposal(scale), []

    def propose(X, rung, walker, step):
        seen.append((len(X), step))
        return inner(X, rung, walker, step)
    cfn = O.make_propose_fn(propose)
    eng = E.Engine(D, Nt, W, seed=seed, swap_rate=sr, add_every_n=N, history_rungs=Nt, history_capacity=cap, map_rungs=Nt)
    try:
        pr.configure(eng, E.PROP_DIAG)
        eng.set_bounds(*bounds); eng.set_prior(*prior); eng.set_target_gaussian(pr.P, pr.like0, mean)
        eng.set_proposal_callback(cfn)
        rng = np.random.default_rng(5)
        x0 = rng.uniform(-1.0, 1.0, size=(Nt * W, D)) * np.sqrt(np.diag(pr.cov))
        eng.set_states(x0)
        lad = O.Ladder(PU.oracle_problem(pr, bounds, prior, mean), pr.beta, W=W, swap_rate=sr, add_every_N=N)
        lad.set_proposals([(O.PROP_DIAG, np.ones(D), 0.0)] * Nt)       # unused
        lad.use_philox(seed)
        lad.enable_history(cap)
        lad.set_host_proposal(cfn)
        lad.set_states(PU.to_oracle_order(x0, Nt, W))

        def compare(e, what):
            PU.assert_same_state(e, lad, what)
            PU.assert_same_history_and_map(e, lad, cap)
        late_rounds(eng, lad, plain_advance(eng, lad), compare)
        # every call was handed the step as it stood: 0..2 young, then 2^32 - 2 .. 2^32 + 4 -- the engine's calls among them (it asks once
        # per sweep for all moving chains; the checker asks chain by chain)
        want = set([0, 1, 2] + [AU.LATE_STEP + k for k in range(CU.AGED_ROUNDS)])
        assert set(st for n, st in seen) == want, sorted(set(st for n, st in seen))
        assert set(st for n, st in seen if n > 1) == want, sorted(set(st for n, st in seen if n > 1))
        assert max(st for n, st in seen) == 2**32 + 4
    finally:
        eng.close()


def test_prior_draw_member_late_in_a_run():
    """TAG_PRIOR: dimension d of a prior draw comes from block d of the chain's stream under tag 4 at the PT step (the lanes kernel, 21
    of 32 lanes; tests/prior_draw_model.py restates the draw)"""
    import prior_draw_cases as PC
    D, Nt, W, cap = 21, 4, 2, 64
    pr0 = PU.problem_for(D, Nt, 1e3)
    prior = ([E.PRIOR_GAUSSIAN] * D, np.zeros(D), 1.5 * np.sqrt(np.diag(pr0.cov)))
    pr, eng, lad, model = PC.mixture_pair(D, Nt, W, E.PROP_LOWER, PC.cum_of([0.3, 0.4, 0.3]), [1.0, 1.0, 0.25], [0.5, 0.0, 0.0], 1, cap=cap, prior=prior)
    try:
        assert eng.sweep_kernel_name == "sweep_lanes_kernel<32, 2, true>", eng.sweep_kernel_name

        def advance(n, sweep):
            (eng.sweep if sweep else eng.step)(n); eng.sync()
            (model.sweep if sweep else model.step)(n)

        def compare(e, what):
            PC.assert_same(e, lad, model, what)
            PC.assert_same_history(e, lad, model, cap)
        moves = []
        late_rounds(eng, lad, lambda n, sweep: (advance(n, sweep), moves.append(int(model.moves.sum()))), compare)
        assert moves[-1] > moves[0] > 0, moves          # the member proposed before and after the ageing
    finally:
        eng.close()


def test_two_rung_shards_in_one_process_late_in_a_run():
    """a ladder of 12 rungs in two engines (ptm_exchange_decide / ptm_exchange_finish_and_sweep, messages by plain copies): both shards'
    exchange kernels replay the ladder's TAG_PT draws at the late step, and the shards together are the checker's whole ladder"""
    import shard_sim
    from box_prefilter_worker import DevShard
    from ptmcmc_amd.parallel import shard_bounds
    D, Nt, W, G, sr = 8, 12, 64, 2, 0.45
    pr, ref, lad = PU.make_pair(D, Nt, W, 1e3, swap_rate=sr)
    x0 = ref.states()
    ref.close()
    shards = []
    try:
        for g in range(G):
            r0, n = shard_bounds(Nt, G, g)
            e = E.Engine(D, Nt, W, swap_rate=sr, rung_begin=r0, rung_count=n)
            pr.configure(e, E.PROP_LOWER)
            e.set_states(x0[r0 * W:(r0 + n) * W])
            shards.append(e)
        lads = shard_sim.build([DevShard(e) for e in shards], halo=4)
        copy = lambda dst, src: dst.copy_from(src.ptr)

        def compare(what):
            assert np.array_equal(np.concatenate([e.states() for e in shards]), PU.to_engine_order(lad.x, Nt, W)), what
            for name in ("llike", "lprior", "ntries", "naccept", "nhist", "last_type"):
                got, want = np.concatenate([getattr(e, name) for e in shards]), PU.to_engine_order(getattr(lad, name), Nt, W)
                assert np.array_equal(got, want), (what, name)
            assert all(e.step_count == lad.step for e in shards), what
        shard_sim.step(lads, copy, 3); lad.pt_step(3)
        compare("young, after 3 PT steps")
        d = AU.largest_shift(max(int(lad.ntries.max()), int(lad.nhist.max())), CU.AGED_ROUNDS)
        for e in shards:
            AU.age_engine(e, AU.LATE_STEP, d)
        AU.age_checker(lad, AU.LATE_STEP, d)
        compare("aged")
        shard_sim.step(lads, copy, 3); lad.pt_step(3)
        compare("aged, after the 3 PT steps across 2^32")
        for e in shards:
            e.sweep(2); e.sync()
        lad.sweep(2)
        compare("aged, after 2 plain sweeps")
        shard_sim.step(lads, copy, 2); lad.pt_step(2)
        compare("aged, after 2 more PT steps")
        t, a = sum(e.swap_counts()[0] for e in shards), sum(e.swap_counts()[1] for e in shards)
        assert np.array_equal(t, lad.swap_count) and np.array_equal(a, lad.swap_accept_count) and a.sum() > 0
        top = max(int(max(e.ntries.max(), e.nhist.max())) for e in shards)
        assert 2**31 - 2**16 < top <= AU.COUNT_MAX - AU.MARGIN, top
    finally:
        for e in shards:
            e.close()


# ---- differential evolution late in a run -----------------------------------------------------------------------------------------
LATE_DE = {
    # the kernel that draws: (D, Nt, W, kind, evolve, options of the pair, the name its PT steps report)
    "sweep_kernel": (7, 3, 64, E.PROP_LOWER, 0.0, dict(time_kernels=True), r"decide_kernel \+ sweep_kernel<8, 2, true, false>"),
    "lanes kernel": (12, 4, 5, E.PROP_LOWER, 0.0, dict(time_kernels=True), r"decide_kernel \+ sweep_lanes_kernel<16, 2, true>"),
    "ladder_steps_kernel": (7, 3, 320, E.PROP_DIAG, 0.0, {}, r"ladder_steps_kernel<8, 1, \d+>"),
    "persistent build 11": (12, 4, 5, E.PROP_LOWER, 0.0, {}, r"ladder_persistent_kernel<16, 0, 11>"),
    "persistent build 15": (12, 4, 5, E.PROP_DENSE, 0.01, {}, r"ladder_persistent_kernel<16, 0, 15>"),
}


@pytest.mark.parametrize("which", sorted(LATE_DE))
def test_differential_evolution_late_in_a_run(which):
    """tests/aging_util.py, late_de_pair: a history stride of 2^24, 128 invented saved rows on both sides, Nhist = 127 * 2^24 - 2 and PT
    step 2^32 - 2 -- row picks, the count of saved rows, readiness, parallel and snooker moves at Nhist ~ 2.1e9; the third step saves a row"""
    import re
    D, Nt, W, kind, ev, kw, kernel = LATE_DE[which]
    pr, eng, lad = AU.late_de_pair(D, Nt, W, kind, evolve=ev, **kw)
    try:
        assert re.fullmatch(kernel, eng.step_kernel_name), eng.step_kernel_name
        AU.run_late_de(eng, lad, evolving=bool(ev))
        if which.startswith("persistent"):
            st = eng.ladder_stats()
            assert st["launches"] > 0 and st["fallbacks"] == 0 and not st["disabled"], st
    finally:
        eng.close()


def test_differential_evolution_on_the_matrix_cores_at_a_late_nhist():
    out = _worker("de_mfma_worker.py", ["late"], {"PTM_DE_MFMA": "1", "PTM_LADDER": "0"})
    assert out.startswith("ok ") and "kernel=de_mfma32_kernel<2,false>" in out, out
    types = set(int(v) for v in out.split("types=")[1].split()[0].split(","))
    assert {0, 10} <= types, out


# ---- found by the aged census --------------------------------------------------------------------------------------------------------
def test_restore_takes_saved_states_as_they_are_under_a_two_sided_reflection():
    """The reference's two-sided reflection folds to a NEGATIVE offset (states.cc:31-45): a state can rest below its lower bound, and a
    second enforce would move it.  ptm_restore must not enforce: the restored engine holds the checkpoint's states and log-priors bit
    for bit and goes on as the checker does.  (Young: the census case whose ageing met it, `ladder_persistent_kernel<16, 0, 27>`.)"""
    name = "ladder_persistent_kernel<16, 0, 27>"
    case = CU.Case(BC.CASES[name], persistent=True)
    eng = case.eng
    try:
        blo, bhi, xmin, xmax = case.space["bounds"]
        dr = [d for d in range(eng.D) if blo[d] == E.BOUND_REFLECT and bhi[d] == E.BOUND_REFLECT]
        assert dr
        case.step(3)
        x = eng.states()
        assert any((x[:, d] < xmin[d]).any() or (x[:, d] > xmax[d]).any() for d in dr), "no state rests outside its reflecting bounds: the case cannot tell"
        ck, lp = eng.checkpoint(), eng.lprior
        eng.restore(ck)
        assert np.array_equal(eng.states(), ck["x"]) and np.array_equal(eng.lprior, lp) and np.array_equal(eng.llike, ck["llike"])
        case.compare("restored")
        case.step(3)
        case.compare("3 PT steps after the restore")
    finally:
        case.close()
