"""Engine-and-checker pairs for the proposal types beyond one Gaussian per rung, shared by the GPU tests: scale mixtures with history
(the persistent ladder kernel's flavours), differential evolution drawn on the device, adaptive proposal sets (with their model,
tests/adaptive_model.py).  Each builds on parity_util.make_pair and hands its further keyword options (bounds, prior, mean, x0,
time_kernels) through to it."""
import numpy as np

import adaptive_model as AM
import parity_util as PU

SEED = 0x5EED0001


def ladder_flavour_pair(D, Nt, W, kind, sr, odf, K, N, cap=64, tmax=1e4, **pair_kw):
    """one-dimensional moves (odf > 0), a scale mixture of K members (K > 0), history and MAP of every N-th add (N > 0)"""
    pr, eng, lad = PU.make_pair(D, Nt, W, tmax, kind=kind, swap_rate=sr, one_d_frac=odf if odf > 0 else None, add_every_n=max(N, 1),
                                history_cap=cap if N else 0, **pair_kw)
    if K:
        rng = np.random.default_rng(K)
        shares = 2.0 ** np.arange(1, K + 1)
        cum = np.tile(np.cumsum(shares) / shares.sum(), (Nt, 1)); cum[:, -1] = 1.0
        scales = np.tile(3.0 ** -np.arange(K)[::-1] * 1.2, (Nt, 1)) * rng.uniform(0.8, 1.2, (Nt, 1))
        odfs = np.tile(np.where(np.arange(K) % 2 == 0, odf, 0.0), (Nt, 1))
        eng.set_proposal_mixture(cum, scales, odfs); lad.set_mixture(cum, scales, odfs)
    return pr, eng, lad


def de_recipe(Nt, K, de_share, odf):
    """the reference sampler's default set (ptmcmc.cc:60-143): differential evolution first, then K Gaussians of doubling shares"""
    g = 2.0 ** np.arange(1, K + 1)
    shares = np.concatenate([[de_share], (1 - de_share) * g / g.sum()])
    cum = np.tile(np.cumsum(shares), (Nt, 1)); cum[:, -1] = 1.0
    scales = np.tile(np.concatenate([[-1.0], 2.0 ** -np.arange(K)[::-1]]), (Nt, 1))
    odfs = np.tile(np.concatenate([[0.0], np.full(K, odf)]), (Nt, 1))
    return cum, scales, odfs


def de_pair(D, Nt, W, kind, N, snooker, ninit, K, cap, de_share=0.7, ignore=0.0, seed=SEED, **pair_kw):
    """differential evolution (ninit x D initial rows in front of the start state) and K Gaussians; history of every N-th add"""
    pr, eng, lad = PU.make_pair(D, Nt, W, 1e3, kind=kind, seed=seed, swap_rate=0.3, add_every_n=N, history_cap=cap, **pair_kw)
    cum, scales, odfs = de_recipe(Nt, K, de_share, 0.5)
    eng.set_proposal_mixture(cum, scales, odfs); lad.set_mixture(cum, scales, odfs)
    rng = np.random.default_rng(D * 1000 + Nt)
    init = None
    if ninit:
        init = rng.uniform(-1.0, 1.0, size=(ninit * D, Nt * W, D)) * np.asarray(pr.halfwidths)[None, None, :] * 0.02
    eng.set_proposal_de(snooker, 0.3, 4.0, ignore, init_rows=init)
    lad.set_de(snooker, 0.3, 4.0, ignore, init_rows=None if init is None else np.stack([PU.to_oracle_order(init[k], Nt, W) for k in range(init.shape[0])]))
    return pr, eng, lad


def doubling(n):
    g = [2.0 ** (k + 1) for k in range(n)]
    t = sum(g)
    return [v / t for v in g]


def one_level(K, odf):
    """K scaled Gaussians of doubling shares: (top shares, leaf scales, leaf oneDfracs)"""
    return doubling(K), [2.0 ** -(K - 1 - k) for k in range(K)], [odf] * K


def adaptive_pair(D, Nt, W, kind, top, scales, odfs, rate, nested=-1, inner=None, rate_in=0.0, cap=0, de=None, ninit=0, evolve=0.0, swap_rate=0.1,
                  **pair_kw):
    """an adaptive proposal set (and its model, which steers the checker) on top of make_pair; de: the snooker share of a
    differential-evolution member with ninit initial rows"""
    pr, eng, lad = PU.make_pair(D, Nt, W, 1e3, kind=kind, seed=SEED, swap_rate=swap_rate, history_cap=cap, **pair_kw)
    K, Ki = len(top), (len(inner) if inner else 0)
    chains = [AM.ChainSet(top, rate, nested, inner, rate_in) for _ in range(Nt * W)]
    w, th, bits, cnt = AM.states_of(chains)
    sc, od = np.tile(scales, (Nt, 1)), np.tile(odfs, (Nt, 1))
    eng.set_proposal_adaptive(K, sc, od, w, th, bits, cnt, nested=nested, K_inner=Ki, rate=rate, rate_inner=rate_in)
    if de is not None:
        init = None
        if ninit:
            rng = np.random.default_rng(D * 100 + Nt)
            init = rng.uniform(-1.0, 1.0, size=(ninit, Nt * W, D)) * np.asarray(pr.halfwidths)[None, None, :] * 0.02
        eng.set_proposal_de(de, 0.3, 4.0, 0.0, init_rows=init)
        lad.set_de(de, 0.3, 4.0, 0.0, init_rows=None if init is None else np.stack([PU.to_oracle_order(init[k], Nt, W) for k in range(ninit)]))
    if evolve:
        eng.set_evolve_temps(evolve); lad.evolve_temps(evolve)
    model = AM.SteeredOracle(lad, SEED, chains, sc, od, de_init_extra=ninit)
    return pr, eng, lad, model


def assert_same_adaptive(eng, lad, model, what):
    """states, scalars, counters, type codes (the model's nested codes) and every chain's adaptive state"""
    Nt, W = eng.Nt, eng.W
    xe, xo = eng.states(), PU.to_engine_order(lad.x, Nt, W)
    assert np.array_equal(xe, xo), "%s: states differ at %s" % (what, np.argwhere(xe != xo)[:4].tolist())
    for name in ("llike", "lprior", "ntries", "naccept", "nhist", "nsize"):
        a, b = getattr(eng, name), PU.to_engine_order(getattr(lad, name), Nt, W)
        assert np.array_equal(a, b), "%s: %s differ at %s" % (what, name, np.argwhere(a != b)[:4].tolist())
    lt = model.last_type()
    assert np.array_equal(eng.last_type, lt), "%s: last_type differ at %s" % (what, np.argwhere(eng.last_type != lt)[:4].tolist())
    st = eng.proposal_adapt_state()
    w, th, bits, cnt = model.state()
    for name, got, want in (("weights", st["weights"], w), ("thresholds", st["thresholds"], th), ("repeat bits", st["repeat_bits"], bits),
                            ("outcomes", st["outcomes"], cnt)):
        assert np.array_equal(got, want), "%s: adaptive %s differ at %s" % (what, name, np.argwhere(got != want)[:4].tolist())


def assert_same_adaptive_history(eng, lad, model, cap):
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
