"""Adaptive proposal sets drawn and adapted ON THE DEVICE (ptm_set_proposal_adaptive) against tests/adaptive_model.py, which restates
proposal_distribution_set's adaptation in plain Python and steers the frozen CPU oracle through it step by step.  Bit for bit:
states, likelihoods, priors, counters, type codes, every saved row, the MAP and every chain's adaptive state."""
import numpy as np
import pytest

import adaptive_model as AM
import oracle_lib as O
import parity_util as PU
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem
from proposal_pairs import (SEED, adaptive_pair as _setup, assert_same_adaptive as _assert_same, assert_same_adaptive_history as _assert_history,
                            doubling as _doubling, one_level as _one_level)

pytestmark = pytest.mark.gpu


def _recipe(de_share=0.8, odf=0.5):
    """the sampler's recipe with --prop_adapt_rate: {differential evolution, a nested set of six Gaussians}"""
    top = [de_share, 1 - de_share]
    inner = _doubling(6)
    scales = [-1.0, 1.0] + [2.0 ** -(5 - k) for k in range(6)]
    odfs = [0.0, 0.0] + [odf] * 6
    return top, inner, scales, odfs


def _run(eng, lad, model, steps, chunks=(1, 7)):
    done = 0
    for n in list(chunks) + [steps - sum(chunks)]:
        eng.step(n); eng.sync(); model.step(n)
        done += n
        _assert_same(eng, lad, model, "after %d steps" % done)


ONE_LEVEL = [
    # D, Nt, W, kind, K, odf, evolve, steps, kernel name prefix
    (6, 8, 3, E.PROP_DIAG, 3, 0.5, 0.0, 90, "sweep_lanes_ada_kernel<8"),          # a lane per dimension
    (12, 6, 2, E.PROP_LOWER, 6, 0.3, 0.01, 110, "sweep_lanes_ada_kernel<16"),     # ... evolving ladder, six members
    (7, 4, 64, E.PROP_LOWER, 3, 0.5, 0.0, 80, "sweep_kernel<8, 2, true, false, true>"),              # general kernel, whole waves per rung
    (5, 3, 64, E.PROP_DIAG, 6, 0.5, 0.01, 110, "sweep_kernel<8, 1, true, false, true>"),             # ... evolving
    (48, 3, 2, E.PROP_DENSE, 3, 0.2, 0.0, 70, "sweep_lanes_ada_kernel<64"),      # 33..64 dimensions: a wave per chain
]


@pytest.mark.parametrize("D,Nt,W,kind,K,odf,ev,steps,kernel", ONE_LEVEL)
def test_one_level_adaptive_set_matches_the_model(D, Nt, W, kind, K, odf, ev, steps, kernel):
    """K scaled Gaussians whose shares adapt at rate 0.3: past 10 K outcomes per chain the bins are rebuilt after every outcome"""
    top, scales, odfs = _one_level(K, odf)
    cap = 2 * steps + 8
    pr, eng, lad, model = _setup(D, Nt, W, kind, top, scales, odfs, 0.3, cap=cap, evolve=ev)
    assert eng.sweep_kernel_name.startswith(kernel), eng.sweep_kernel_name
    assert "persistent" not in eng.step_kernel_name and "ladder_steps" not in eng.step_kernel_name, eng.step_kernel_name
    _run(eng, lad, model, steps)
    _assert_history(eng, lad, model, cap)
    assert min(c.top.count for c in model.chains) > 10 * K   # (the every-outcome rebuild was reached)
    st = eng.proposal_adapt_state()
    assert not np.array_equal(st["weights"][0], top)
    assert np.allclose(st["weights"].sum(axis=1), 1.0)
    eng.close()


@pytest.mark.parametrize("more", [False, True])
@pytest.mark.parametrize("D,Nt,W,kind,ninit", [(3, 6, 2, E.PROP_DIAG, 0), (12, 4, 64, E.PROP_LOWER, 10)])
def test_the_samplers_adaptive_recipe_with_differential_evolution(D, Nt, W, kind, ninit, more):
    """{differential evolution 0.8, a nested set of six Gaussians} -- the top set adapts only with --prop_adapt_more.  Differential
    evolution is drawn on the device from the history (no initial rows: passed over until 10 D rows are saved)."""
    top, inner, scales, odfs = _recipe()
    steps = 100
    cap = 2 * steps + 8
    rate = 0.3
    pr, eng, lad, model = _setup(D, Nt, W, kind, top, scales, odfs, rate if more else 0.0, nested=1, inner=inner, rate_in=rate, cap=cap,
                                 de=0.2, ninit=ninit * D)
    assert eng.sweep_kernel_name.startswith("sweep_lanes_ada_kernel<"), eng.sweep_kernel_name
    _run(eng, lad, model, steps)
    _assert_history(eng, lad, model, cap)
    lt = set(int(v) for v in np.unique(eng.last_type))
    assert (0 in lt or 10 in lt) and any(v % 10 == 1 and v >= 1 for v in lt), lt
    st = eng.proposal_adapt_state()
    assert (st["outcomes"][:, 0].max() > 0) == more
    assert st["outcomes"][:, 1].max() > 0
    eng.close()


def test_a_host_callback_likelihood_with_an_adaptive_set():
    """the plug-in likelihood's propose and accept passes (the accept pass picks again and adapts): the toy LISA problem"""
    import lisa_toy
    D, Nt, W, steps = 6, 10, 2, 80
    beta = E.geometric_ladder(Nt, 1e4)
    rng = np.random.default_rng(5)
    lo = np.array(lisa_toy.CENTERS) - np.array(lisa_toy.SCALES)
    hi = np.array(lisa_toy.CENTERS) + np.array(lisa_toy.SCALES)
    x0 = rng.uniform(lo + 0.05, hi - 0.05, size=(Nt * W, D))
    fac = np.tile(np.array(lisa_toy.SCALES) / 100.0, (Nt, 1))
    eng = E.Engine(D, Nt, W, swap_rate=0.1, seed=SEED)
    eng.set_bounds(lisa_toy.BLO, lisa_toy.BHI, lisa_toy.BMIN, lisa_toy.BMAX)
    eng.set_prior(lisa_toy.TYPES, lisa_toy.CENTERS, lisa_toy.SCALES)
    eng.set_target_callback(lisa_toy.loglike)
    eng.set_ladder(beta)
    eng.set_proposals(E.PROP_DIAG, fac)
    eng.set_states(x0)
    pb = O.Problem(D)
    pb.set_bounds(lisa_toy.BLO, lisa_toy.BHI, lisa_toy.BMIN, lisa_toy.BMAX)
    pb.set_prior(lisa_toy.TYPES, lisa_toy.CENTERS, lisa_toy.SCALES)
    pb.set_user(lisa_toy.loglike)
    lad = O.Ladder(pb, beta, W=W, swap_rate=0.1)
    lad.set_proposals([(O.PROP_DIAG, fac[r], 0.0) for r in range(Nt)])
    lad.use_philox(SEED)
    lad.set_states(PU.to_oracle_order(x0, Nt, W))
    top, scales, odfs = [0.5, 0.5], [1.0, 1.0], [0.0, 0.0]
    inner = _doubling(4)
    scales = [4.0, 1.0] + [2.0 ** -k for k in range(4)]
    odfs = [0.5, 0.0] + [0.5] * 4
    chains = [AM.ChainSet(top, 0.3, 1, inner, 0.3) for _ in range(Nt * W)]
    w, th, bits, cnt = AM.states_of(chains)
    sc, od = np.tile(scales, (Nt, 1)), np.tile(odfs, (Nt, 1))
    eng.set_proposal_adaptive(2, sc, od, w, th, bits, cnt, nested=1, K_inner=4, rate=0.3, rate_inner=0.3)
    model = AM.SteeredOracle(lad, SEED, chains, sc, od)
    assert eng.sweep_kernel_name.startswith("sweep_lanes_ada_kernel<8"), eng.sweep_kernel_name
    _run(eng, lad, model, steps)
    assert min(c.top.count for c in chains) > 20
    eng.close()


@pytest.mark.parametrize("D,Nt,W,kind,before", [(6, 64, 1, E.PROP_DIAG, "ladder_persistent_kernel"), (32, 2, 320, E.PROP_LOWER, "sweep_mfma32_kernel")])
def test_adaptive_engines_keep_off_the_persistent_and_matrix_core_kernels(D, Nt, W, kind, before):
    top, scales, odfs = _one_level(3, 0.5)
    pr, eng, lad = PU.make_pair(D, Nt, W, 1e3, kind=kind, seed=SEED)
    assert before in eng.step_kernel_name, eng.step_kernel_name   # (what the engine takes without the adaptive set)
    eng.close()
    pr, eng, lad, model = _setup(D, Nt, W, kind, top, scales, odfs, 0.3)
    name = eng.step_kernel_name
    assert name.startswith("decide_kernel + sweep_lanes_ada_kernel<") or (name.startswith("decide_kernel + sweep_kernel<") and name.endswith(", false, true>")), name
    _run(eng, lad, model, 50 if W > 1 else 80)
    eng.close()


@pytest.mark.parametrize("D,Nt,W", [(6, 8, 3), (6, 12, 1), (7, 4, 64)])
def test_rate_zero_is_the_fixed_mixture(D, Nt, W):
    """rate 0 through ptm_set_proposal_adaptive: the same chains, bit for bit, as ptm_set_proposal_mixture with the same shares"""
    top, scales, odfs = _one_level(4, 0.5)
    chains = [AM.ChainSet(top, 0.0) for _ in range(Nt * W)]
    w, th, bits, cnt = AM.states_of(chains)
    runs = []
    for ada in (False, True):
        pr, eng, lad = PU.make_pair(D, Nt, W, 1e3, kind=E.PROP_DIAG, seed=SEED)
        if ada:
            eng.set_proposal_adaptive(4, np.tile(scales, (Nt, 1)), np.tile(odfs, (Nt, 1)), w, th, bits, cnt)
        else:
            eng.set_proposal_mixture(np.tile(th[0], (Nt, 1)), np.tile(scales, (Nt, 1)), np.tile(odfs, (Nt, 1)))
        eng.step(60); eng.sync()
        runs.append((eng.states(), eng.llike, eng.last_type, eng.naccept))
        if ada:
            st = eng.proposal_adapt_state()
            assert np.array_equal(st["weights"], w) and np.array_equal(st["thresholds"], th) and not st["outcomes"].any()
        eng.close()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_a_snapshot_of_states_and_adapt_state_continues_the_run():
    D, Nt, W = 6, 8, 3
    top, inner, scales, odfs = _recipe(0.0)
    top = [0.3, 0.7]
    scales[0], odfs[0] = 3.0, 0.5   # (no differential evolution: a Gaussian member beside the nested set)
    pr, eng, lad, model = _setup(D, Nt, W, E.PROP_DIAG, top, scales, odfs, 0.3, nested=1, inner=inner, rate_in=0.3)
    eng.step(50); eng.sync()
    ck, st = eng.checkpoint(), eng.proposal_adapt_state()
    eng.step(50); eng.sync()
    want = (eng.states(), eng.last_type, eng.proposal_adapt_state())
    # a second engine, set up the same way with a different initial adaptive state, then restored
    pr2, eng2, lad2, model2 = _setup(D, Nt, W, E.PROP_DIAG, [0.5, 0.5], scales, odfs, 0.3, nested=1, inner=inner, rate_in=0.3)
    eng2.restore(ck)
    eng2.set_proposal_adapt_state(st["weights"], st["thresholds"], st["repeat_bits"], st["outcomes"])
    eng2.step(50); eng2.sync()
    assert np.array_equal(eng2.states(), want[0]) and np.array_equal(eng2.last_type, want[1])
    got = eng2.proposal_adapt_state()
    for k in got:
        assert np.array_equal(got[k], want[2][k]), k
    eng.close(); eng2.close()


def test_two_engines_split_by_walkers_equal_one():
    D, Nt, W = 6, 6, 4
    top, scales, odfs = _one_level(3, 0.5)
    pr, eng, lad, model = _setup(D, Nt, W, E.PROP_DIAG, top, scales, odfs, 0.3)
    x0 = eng.states()
    eng.step(70); eng.sync()
    whole = (eng.states().reshape(Nt, W, D), eng.proposal_adapt_state())
    chains = [AM.ChainSet(top, 0.3) for _ in range(Nt * 2)]
    w, th, bits, cnt = AM.states_of(chains)
    for w0 in (0, 2):
        e = E.Engine(D, Nt, 2, seed=SEED, swap_rate=0.1, walker_begin=w0)
        pr.configure(e, E.PROP_DIAG)
        e.set_states(x0.reshape(Nt, W, D)[:, w0:w0 + 2].reshape(Nt * 2, D))
        e.set_proposal_adaptive(3, np.tile(scales, (Nt, 1)), np.tile(odfs, (Nt, 1)), w, th, bits, cnt, rate=0.3)
        e.step(70); e.sync()
        assert np.array_equal(e.states().reshape(Nt, 2, D), whole[0][:, w0:w0 + 2])
        st = e.proposal_adapt_state()
        for k in st:
            assert np.array_equal(st[k].reshape(Nt, 2, -1), whole[1][k].reshape(Nt, W, -1)[:, w0:w0 + 2]), k
        e.close()
    eng.close()


def test_refused_configurations_leave_the_earlier_one_working():
    D, Nt, W = 6, 6, 2
    top, inner, scales, odfs = _recipe()
    top = [0.4, 0.6]
    scales[0], odfs[0] = 2.0, 0.0
    pr, eng, lad, model = _setup(D, Nt, W, E.PROP_DIAG, top, scales, odfs, 0.3, nested=1, inner=inner, rate_in=0.3)
    eng.step(20); eng.sync(); model.step(20)
    w, th, bits, cnt = model.state()
    sc, od = np.tile(scales, (Nt, 1)), np.tile(odfs, (Nt, 1))
    good = dict(K=2, scales=sc, one_d_fracs=od, weights=w, thresholds=th, repeat_bits=bits, outcomes=cnt, nested=1, K_inner=6, rate=0.3, rate_inner=0.3)

    def bad(**kw):
        a = dict(good); a.update(kw)
        return a
    neg2 = sc.copy(); neg2[:, 2] = -1.0; neg2[:, 0] = -1.0         # a negative scale inside the nested set
    two = np.tile([-1.0, -1.0, 1.0], (Nt, 1))
    nan = sc.copy(); nan[1, 3] = np.nan
    wneg = w.copy(); wneg[0, 0] = -0.1
    wzero = w.copy(); wzero[0, 2:] = 0.0
    thdec = th.copy(); thdec[0, 2], thdec[0, 3] = thdec[0, 3], thdec[0, 2]
    thlast = th.copy(); thlast[1, 1] = 0.999
    cases = [bad(K=0), bad(K=9), bad(nested=2), bad(nested=-2), bad(K_inner=0), bad(K_inner=9), bad(rate=1.0), bad(rate_inner=-0.1),
             bad(scales=neg2), bad(scales=nan), bad(one_d_fracs=od + 2.0), bad(weights=wneg), bad(weights=wzero), bad(thresholds=thdec),
             bad(thresholds=thlast),
             dict(K=3, scales=two, one_d_fracs=np.zeros((Nt, 3)), weights=np.full((Nt * W, 3), 1 / 3), thresholds=np.tile([1 / 3, 2 / 3, 1.0], (Nt * W, 1)),
                  repeat_bits=np.full((Nt * W, 2), 7), outcomes=np.zeros((Nt * W, 2))),   # two negatives
             dict(K=2, scales=np.tile([1.0, -1.0], (Nt, 1)), one_d_fracs=np.zeros((Nt, 2)), weights=np.full((Nt * W, 2), 0.5),
                  thresholds=np.tile([0.5, 1.0], (Nt * W, 1)), repeat_bits=np.full((Nt * W, 2), 3), outcomes=np.zeros((Nt * W, 2)))]   # DE last
    import ctypes as C
    for a in cases:   # (straight into the C ABI: the set's shape is checked before any array is read)
        arr = lambda v, t: np.ascontiguousarray(v, dtype=t)
        keep = [arr(a["scales"], np.float64), arr(a["one_d_fracs"], np.float64), arr(a["weights"], np.float64), arr(a["thresholds"], np.float64),
                arr(a["repeat_bits"], np.int32), arr(a["outcomes"], np.int32)]
        q = E.PtmAdaptiveSet(a["K"], a.get("nested", -1), a.get("K_inner", 0), a.get("rate", 0.3), a.get("rate_inner", 0.0))
        rc = eng.L.ptm_set_proposal_adaptive(eng.h, C.byref(q), *[k.ctypes.data_as(E._dp) for k in keep[:4]], *[k.ctypes.data_as(E._i32p) for k in keep[4:]])
        assert rc == -1, (rc, a["K"], E.load().ptm_last_error())
    with pytest.raises(E.PtmError):
        eng.set_proposal_adapt_state(wneg, th, bits, cnt)
    _run(eng, lad, model, 30, chunks=(3,))
    eng.close()
    # a rung shard
    e = E.Engine(D, Nt, W, rung_begin=0, rung_count=3)
    e.set_ladder(pr.beta)
    e.set_proposals(E.PROP_DIAG, np.ones((3, D)))
    with pytest.raises(E.PtmError, match="rung shard"):
        e.set_proposal_adaptive(**dict(good, scales=sc[:3], one_d_fracs=od[:3], weights=w[:6], thresholds=th[:6], repeat_bits=bits[:6], outcomes=cnt[:6]))
    e.close()


def test_a_fixed_mixture_switches_adaptation_off():
    D, Nt, W = 6, 6, 2
    top, scales, odfs = _one_level(3, 0.5)
    pr, eng, lad, model = _setup(D, Nt, W, E.PROP_DIAG, top, scales, odfs, 0.3)
    assert eng.sweep_kernel_name.startswith("sweep_lanes_ada_kernel<")
    eng.set_proposal_mixture(np.tile([0.2, 0.5, 1.0], (Nt, 1)), np.tile(scales, (Nt, 1)), np.tile(odfs, (Nt, 1)))
    assert eng.sweep_kernel_name.startswith("sweep_lanes_kernel<"), eng.sweep_kernel_name
    with pytest.raises(E.PtmError, match="no adaptive"):
        eng.proposal_adapt_state()
    eng.close()


def test_an_adaptive_set_keeps_the_target():
    """moments of a correlated Gaussian target at rate 0.3 (tests/test_gpu_statistics.py's criterion)"""
    D, Nt, W, nsnap, spacing = 8, 6, 1024, 12, 100
    rng = np.random.default_rng(31)
    pr = GaussianProblem(D, Nt, 1e2)
    eng = E.Engine(D, Nt, W, swap_rate=0.2, seed=0xADA)
    pr.configure(eng, E.PROP_LOWER)
    top, scales, odfs = _one_level(4, 0.5)
    chains = [AM.ChainSet(top, 0.3) for _ in range(Nt * W)]
    w, th, bits, cnt = AM.states_of(chains)
    eng.set_proposal_adaptive(4, np.tile(scales, (Nt, 1)), np.tile(odfs, (Nt, 1)), w, th, bits, cnt, rate=0.3)
    L = np.linalg.cholesky(pr.cov)
    z = rng.standard_normal((Nt, W, D))
    eng.set_states(((z @ L.T) / np.sqrt(np.asarray(pr.beta))[:, None, None]).reshape(Nt * W, D))
    acc = np.zeros((Nt, D, D))
    for k in range(nsnap):
        eng.step(spacing); eng.sync()
        X = eng.states().reshape(Nt, W, D)
        acc += np.einsum("rwi,rwj->rij", X, X)
    n = nsnap * W
    bound = 5.0 * np.sqrt(2.0 / (n / 2.0))
    errs = []
    for r in range(Nt // 2):
        C = acc[r] / n
        want = pr.cov / pr.beta[r]
        s = np.sqrt(np.diag(want))
        errs.append(np.abs((C - want) / np.outer(s, s)).max())
    assert max(errs) < bound, (errs, bound)
    tries, acc_ = eng.ntries.sum() - eng.Nc, eng.naccept.sum() - eng.Nc
    assert 0.05 * tries < acc_ < 0.95 * tries
    assert not np.allclose(eng.proposal_adapt_state()["weights"], top)
    eng.close()
