"""ptm_log_evidence on the device against tests/evidence_model.py on the engine's own ring -- log_evidence, up, down and count bit for
bit --, its refusals, and the estimator's value on a target whose tempered means are known."""
import math

import numpy as np
import pytest

import evidence_model as M
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem

pytestmark = pytest.mark.gpu


def ladder(Nt, W, steps, cap, add_every_n=1, swap_rate=0.1, evolve=0.0, D=2, seed=0xE71D):
    pr = GaussianProblem(D, Nt, 1e2)
    eng = E.Engine(D, Nt, W, swap_rate=swap_rate, seed=seed, add_every_n=add_every_n, history_rungs=Nt, history_capacity=cap)
    pr.configure(eng, E.PROP_LOWER)
    if evolve > 0:
        eng.set_evolve_temps(evolve)
    eng.init_from_prior()
    if steps:
        eng.step(steps)
        eng.sync()
    return eng


def same(a, b):
    """the same doubles, bit for bit (an empty window's 0 / 0 is a NaN on both sides)"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return a.shape == b.shape and all((math.isnan(x) and math.isnan(y)) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check_against_model(eng, ilen, add_every_n):
    ev, up, down, count = eng.log_evidence(ilen)
    h = eng.history()
    nhist, beta = eng.nhist, eng.invtemps()
    for w in range(eng.W):
        m_ev, m_up, m_down, m_count = M.ring_total(h["llike"], h["row"], nhist, beta[w], eng.Nt, eng.W, w, ilen, add_every_n)
        assert list(count[:, w]) == m_count, (w, count[:, w], m_count)
        assert same(up[:, w], m_up), (w, up[:, w], m_up)
        assert same(down[:, w], m_down), (w, down[:, w], m_down)
        assert same(ev[w], m_ev), (w, ev[w], m_ev)
    return ev, up, down, count, nhist


# Nt, W, add_every_n, swap_rate, steps, ilen (no multiple of add_every_n where that is 3)
SHAPES = [(2, 1, 1, 0.1, 300, 200), (3, 5, 3, 0.1, 400, 250), (9, 70, 1, 0.4, 300, 200), (9, 70, 3, 0.4, 300, 200)]


@pytest.mark.parametrize("Nt,W,a,swap_rate,steps,ilen", SHAPES, ids=["Nt2_W1", "Nt3_W5_every3", "Nt9_W70", "Nt9_W70_every3"])
def test_device_equals_the_model_on_the_engines_ring(Nt, W, a, swap_rate, steps, ilen):
    eng = ladder(Nt, W, steps, cap=2 * steps + 4, add_every_n=a, swap_rate=swap_rate)
    ev, up, down, count, nhist = check_against_model(eng, ilen, a)
    assert np.isfinite(ev).all() and (count > 0).all()
    if W >= 64:   # a rung exchanged twice in a step makes one more add_state call: the walkers of a rung differ
        assert any(len(set(nhist.reshape(Nt, W)[r])) > 1 for r in range(1, Nt - 1))
    eng.close()


def test_a_wrapped_ring_that_still_holds_the_window():
    a, ilen = 1, 150
    eng = ladder(4, 6, 500, cap=ilen // a + 2, add_every_n=a, swap_rate=0.3)
    assert eng.nsize.min() > eng.hist_cap                     # wrapped
    ev, _, _, count, _ = check_against_model(eng, ilen, a)
    assert np.isfinite(ev).all() and (count == ilen - 1).all()
    eng.close()


def test_a_ring_that_lost_the_window_is_refused_and_the_outputs_stay():
    eng = ladder(4, 6, 500, cap=100, swap_rate=0.3)
    out = (np.full(6, 7.25), np.full((3, 6), -3.5), np.full((3, 6), 11.0), np.full((4, 6), 99, dtype=np.int32))
    with pytest.raises(E.PtmError) as ei:
        eng.log_evidence(200, out=out)
    assert "ptm error -1" in str(ei.value) and "history_capacity must hold the evidence window" in str(ei.value)
    assert (out[0] == 7.25).all() and (out[1] == -3.5).all() and (out[2] == 11.0).all() and (out[3] == 99).all()
    eng.close()


def test_a_window_longer_than_the_run_is_empty():
    eng = ladder(3, 5, 40, cap=200)
    ev, up, down, count = eng.log_evidence(5000)
    assert (count == 0).all() and np.isnan(ev).all() and np.isnan(up).all() and np.isnan(down).all()
    check_against_model(eng, 5000, 1)
    eng.close()


def test_an_evolving_ladder_uses_every_walkers_own_temperatures():
    eng = ladder(5, 3, 400, cap=900, swap_rate=0.3, evolve=0.01)
    beta = eng.invtemps()
    assert not np.array_equal(beta[0], beta[1])
    ev, _, _, _, _ = check_against_model(eng, 300, 1)
    assert np.isfinite(ev).all()
    eng.close()


def test_refusals():
    pr = GaussianProblem(2, 4, 1e2)
    eng = E.Engine(2, 4, 2)                                   # no ring
    pr.configure(eng, E.PROP_LOWER); eng.init_from_prior()
    with pytest.raises(E.PtmError) as ei:
        eng.log_evidence(10)
    assert "ptm error -1" in str(ei.value) and "no history" in str(ei.value)
    eng.close()
    eng = E.Engine(2, 4, 2, history_rungs=2, history_capacity=50)
    pr.configure(eng, E.PROP_LOWER); eng.init_from_prior()
    with pytest.raises(E.PtmError) as ei:
        eng.log_evidence(10)
    assert "ptm error -1" in str(ei.value) and "history_rungs" in str(ei.value)
    with pytest.raises(E.PtmError) as ei:
        eng.log_evidence(0)
    assert "ptm error -1" in str(ei.value) and "ilen" in str(ei.value)
    eng.close()
    eng = E.Engine(2, 4, 2, rung_begin=0, rung_count=2, history_rungs=1, history_capacity=50)   # a rung shard
    with pytest.raises(E.PtmError) as ei:
        eng.log_evidence(10)
    assert "ptm error -2" in str(ei.value) and "rung shard" in str(ei.value)
    eng.close()


def test_the_call_leaves_the_chains_alone():
    a, b = ladder(6, 8, 150, cap=400, swap_rate=0.3), ladder(6, 8, 150, cap=400, swap_rate=0.3)
    a.log_evidence(100)
    for e in (a, b):
        e.step(150)
        e.sync()
    a.log_evidence(100)
    assert np.array_equal(a.states(), b.states()) and np.array_equal(a.llike, b.llike) and np.array_equal(a.nhist, b.nhist)
    assert np.array_equal(a.history()["llike"], b.history()["llike"])
    a.close(); b.close()


def test_the_estimate_of_a_gaussian_target_is_the_estimator_of_its_analytic_means():
    """A 4-D unit Gaussian in a box of +-40 (ten standard deviations of the hottest rung: no truncation to speak of), Nt = 8,
    Tmax = 16, W = 64, every chain started from an exact sample of its tempered target, 2000 steps, ilen = 2000.  Under beta the
    mean of lnL is like0 - D / (2 beta); the expected value is the SAME estimator -- the trapezoid over the ladder and the
    extrapolation below the hottest rung -- applied to those means (not the exact ln Z: the trapezoid's bias is the estimator's).
    The estimator is linear in the llikes and the chains are stationary, so the mean over the walkers estimates exactly that; the
    standard error is the walkers' own spread / sqrt(64) (they are independent ladders), the bound 5 of them."""
    D, Nt, W, steps = 4, 8, 64, 2000
    pr = GaussianProblem(D, Nt, 16.0)
    pr.cov = np.eye(D); pr.P = np.eye(D); pr.like0 = -0.5 * D * math.log(2 * math.pi); pr.halfwidths = np.full(D, 40.0)
    eng = E.Engine(D, Nt, W, swap_rate=0.2, seed=0xE71DE, history_rungs=Nt, history_capacity=2 * steps + 4)
    pr.configure(eng, E.PROP_LOWER)
    rng = np.random.default_rng(2024)
    beta = np.asarray(pr.beta)
    eng.set_states((rng.standard_normal((Nt, W, D)) / np.sqrt(beta)[:, None, None]).reshape(Nt * W, D))
    eng.step(steps)
    eng.sync()
    ev, up, down, count = eng.log_evidence(steps)
    assert (count >= steps - 1).all() and np.isfinite(ev).all()
    mean_ll = pr.like0 - D / (2 * beta)
    want = 0.0
    for i in range(Nt - 1):
        u, d = mean_ll[i + 1] * (beta[i] - beta[i + 1]), -mean_ll[i] * (beta[i + 1] - beta[i])
        want += (u + d) / 2.0
    want += (u + d) / 2.0 / (beta[Nt - 2] / beta[Nt - 1] - 1)
    se = ev.std(ddof=1) / math.sqrt(W)
    print("log-evidence: mean over %d walkers %.5f, the estimator of the analytic means %.5f, standard error %.5f (%.2f of them); exact ln Z = %.5f"
          % (W, ev.mean(), want, se, (ev.mean() - want) / se, -D * math.log(80.0)))
    assert se > 0
    assert abs(ev.mean() - want) < 5 * se
    t, acc = eng.swap_counts()
    assert acc.sum() > 0.05 * t.sum() and eng.naccept.sum() - eng.Nc > 0.05 * (eng.ntries.sum() - eng.Nc)
    eng.close()
