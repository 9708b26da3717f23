"""Child process of tests/test_gpu_device_likelihood.py: user likelihoods written in torch, run by the engine ON THE DEVICE
(ptm_set_target_device), against the CPU oracle and against the host-callback path.

torch is imported FIRST (tests/torch_shard_worker.py says why: one HIP runtime per process).  Usage: device_like_worker.py CASE [ARGS..];
prints "OK <case>" on success, raises (non-zero exit) otherwise."""
import json
import math
import os
import sys

import torch  # noqa: E402  (before anything loads libptm_engine.so)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np

import lisa_toy
import oracle_lib as O
import parity_util as PU
from ptmcmc_amd import engine as E

DEV = torch.device("cuda", 0)
SUFFIX = " + device likelihood"


# -- a polynomial likelihood whose torch and numpy forms give the same bits: + - * only, one elementwise op per kernel, the
#    columns summed in a Python loop over d in the same order
def poly_coefs(D, seed=3):
    rng = np.random.default_rng(seed)
    return [float(v) for v in rng.uniform(-0.5, 0.5, D)], [float(-0.5 * v) for v in rng.uniform(0.5, 2.0, D)]


def poly_numpy(c, k, cut=None):
    def f(x):
        if cut is not None:
            if float(x[0]) > cut[0]:
                return -math.inf
            if float(x[1]) > cut[1]:
                return math.nan
        acc = 0.0
        for d in range(len(c)):
            t = float(x[d]) - c[d]
            t = t * t
            t = t * k[d]
            acc = acc + t
        return acc
    return f


def poly_torch(c, k, cut=None):
    def f(X, count, out):
        acc = torch.zeros(X.shape[0], dtype=torch.float64, device=X.device)
        for d in range(len(c)):
            t = X[:, d] - c[d]
            t = t * t
            t = t * k[d]
            acc = acc + t
        if cut is not None:
            acc = torch.where(X[:, 1] > cut[1], torch.full_like(acc, math.nan), acc)
            acc = torch.where(X[:, 0] > cut[0], torch.full_like(acc, -math.inf), acc)
        out.copy_(acc)
    return f


# -- the toy LISA likelihood (exampleLISA.cc:59-72,130-142) in torch: transcendental functions, the same on both paths only
#    because both paths run THIS function on the device
def lisa_torch(X, count, out):
    d, phi, inc, lam, beta, psi = (X[:, j] for j in range(6))
    P3 = math.pi / 3
    ap = 0.75 * (3 - torch.cos(2 * beta)) * torch.cos(2 * lam - P3)       # a_plus = i * ap
    ac = 3.0 * torch.sin(beta) * torch.sin(2 * lam - P3)                   # a_cross = i * ac
    ep = -0.75 * (3 - torch.cos(2 * beta)) * torch.sin(2 * lam - P3)      # e_plus = i * ep
    ec = 3.0 * torch.sin(beta) * torch.cos(2 * lam - P3)                   # e_cross = i * ec
    pref = 0.5 / d * math.sqrt(5 / math.pi)
    c4, s4 = torch.cos(inc / 2) ** 4, torch.sin(inc / 2) ** 4
    def modes(plus_i, cross_i):
        plus = torch.complex(torch.zeros_like(plus_i), plus_i)
        cross = torch.complex(torch.zeros_like(cross_i), cross_i)
        m22 = (pref * c4) * torch.exp(torch.complex(torch.zeros_like(phi), 2 * (-phi - psi))) * 0.5 * (plus + 1j * cross)
        m2m2 = (pref * s4) * torch.exp(torch.complex(torch.zeros_like(phi), 2 * (-phi + psi))) * 0.5 * (plus - 1j * cross)
        return m22 + m2m2
    sa, se = modes(ap, ac), modes(ep, ec)
    r = -0.5 * lisa_toy.FACTOR * (torch.abs(sa - lisa_toy.SA_INJ) ** 2 + torch.abs(se - lisa_toy.SE_INJ) ** 2)
    out.copy_(r)


def host_of(tfn, D):
    """a torch device function wrapped as a host batch callback: numpy -> device -> the function -> numpy"""
    def f(X):
        Xt = torch.as_tensor(np.ascontiguousarray(X), dtype=torch.float64, device=DEV)
        out = torch.empty(Xt.shape[0], dtype=torch.float64, device=DEV)
        cnt = torch.full((1,), Xt.shape[0], dtype=torch.int32, device=DEV)
        tfn(Xt, cnt, out)
        return out.cpu().numpy()
    return f


def check_name(eng, start=None):
    nm = eng.step_kernel_name
    assert nm.endswith(SUFFIX), nm
    assert nm.startswith("decide_kernel + "), nm
    if start:
        assert eng.sweep_kernel_name.startswith(start), eng.sweep_kernel_name


# ---------------------------------------------------------------------------------------------------------- oracle parity
def case_c5(Nt, W, ev, cut=False):
    """BASELINE configs[4]'s shape (test_host_callback_likelihood_C5_exampleLISA) with a device likelihood"""
    D = 6
    beta = E.geometric_ladder(Nt, 1e9)
    rng = np.random.default_rng(4)
    lo = np.array(lisa_toy.CENTERS) - np.array(lisa_toy.SCALES)
    hi = np.array(lisa_toy.CENTERS) + np.array(lisa_toy.SCALES)
    x0 = rng.uniform(lo + 0.05, hi - 0.05, size=(Nt * W, D))
    sig = np.array(lisa_toy.SCALES) / 20.0
    c, k = poly_coefs(D)
    k = [v * 40.0 for v in k]
    cuts = (2.2, 4.0) if cut else None
    eng = E.Engine(D, Nt, W, swap_rate=0.3)
    eng.set_bounds(lisa_toy.BLO, lisa_toy.BHI, lisa_toy.BMIN, lisa_toy.BMAX)
    eng.set_prior(lisa_toy.TYPES, lisa_toy.CENTERS, lisa_toy.SCALES)
    eng.set_target_device(poly_torch(c, k, cuts))
    eng.set_ladder(beta)
    fac = np.tile(sig, (Nt, 1)) / np.sqrt(beta)[:, None].clip(1e-3)
    eng.set_proposals(E.PROP_DIAG, fac, np.full(Nt, 0.5))
    if cut:   # start states inside the likelihood's support
        x0[:, 0] = np.minimum(x0[:, 0], 2.0); x0[:, 1] = np.minimum(x0[:, 1], 3.9)
    eng.set_states(x0)
    pb = O.Problem(D)
    pb.set_bounds(lisa_toy.BLO, lisa_toy.BHI, lisa_toy.BMIN, lisa_toy.BMAX)
    pb.set_prior(lisa_toy.TYPES, lisa_toy.CENTERS, lisa_toy.SCALES)
    pb.set_user(poly_numpy(c, k, cuts))
    lad = O.Ladder(pb, beta, W=W, swap_rate=0.3)
    lad.set_proposals([(O.PROP_DIAG, fac[r], 0.5) for r in range(Nt)])
    lad.use_philox(0x5EED0001)
    lad.set_states(PU.to_oracle_order(x0, Nt, W))
    if ev:
        eng.set_evolve_temps(ev); lad.evolve_temps(ev)
    check_name(eng)
    PU.assert_same_state(eng, lad, "start")
    for s in range(6):
        eng.step(5); eng.sync(); lad.pt_step(5)
        PU.assert_same_state(eng, lad, "after %d steps" % (5 * (s + 1)))
        assert np.array_equal(eng.invtemps(), lad.betaw)
    assert eng.naccept.sum() - eng.Nc > 50
    if cut:
        assert eng.ntries.sum() - eng.Nc > eng.naccept.sum() - eng.Nc
    eng.close()


def _recipe(Nt, K, de_share, odf):
    g = 2.0 ** np.arange(1, K + 1)
    shares = np.concatenate([[de_share], (1 - de_share) * g / g.sum()])
    cum = np.tile(np.cumsum(shares), (Nt, 1)); cum[:, -1] = 1.0
    scales = np.tile(np.concatenate([[-1.0], 2.0 ** -np.arange(K)[::-1]]), (Nt, 1))
    odfs = np.tile(np.concatenate([[0.0], np.full(K, odf)]), (Nt, 1))
    return cum, scales, odfs


def case_recipe(D, Nt, W, kind, steps, ev, de_share, K, ninit, start=None, seed=0x5EED0001):
    """the sampler's default recipe with a device likelihood: differential evolution from the device's history ring + K Gaussians,
    evolving ladder, history, MAP -- states, counters, every saved row, MAPs and temperatures against the oracle"""
    cap = 2 * steps + 8
    pr = PU.problem_for(D, Nt, 1e3)
    c, k = poly_coefs(D, seed=D)
    k = [v / (np.asarray(pr.halfwidths)[d] * 0.05) ** 2 for d, v in enumerate(k)]
    eng = E.Engine(D, Nt, W, seed=seed, swap_rate=0.3, history_rungs=Nt if cap else 0, history_capacity=cap, map_rungs=Nt if cap else 0)
    fac = pr.configure(eng, kind)
    eng.init_from_prior()
    x0 = eng.states()
    eng.set_target_device(poly_torch(c, k))
    pb = PU.oracle_problem(pr)
    pb.set_user(poly_numpy(c, k))
    lad = O.Ladder(pb, pr.beta, W=W, swap_rate=0.3)
    lad.set_proposals([(PU.KIND_TO_ORACLE[kind], fac[r], 0.0) for r in range(Nt)])
    lad.use_philox(seed)
    lad.enable_history(cap)
    eng.set_states(x0)
    lad.set_states(PU.to_oracle_order(x0, Nt, W))
    if K:
        cum, scales, odfs = _recipe(Nt, K, de_share, 0.5)
        eng.set_proposal_mixture(cum, scales, odfs); lad.set_mixture(cum, scales, odfs)
        rng = np.random.default_rng(D * 1000 + Nt)
        init = rng.uniform(-1.0, 1.0, size=(ninit * D, Nt * W, D)) * np.asarray(pr.halfwidths)[None, None, :] * 0.02 if ninit else None
        eng.set_proposal_de(0.1, 0.3, 4.0, 0.0, init_rows=init)
        lad.set_de(0.1, 0.3, 4.0, 0.0, init_rows=None if init is None else np.stack([PU.to_oracle_order(init[j], Nt, W) for j in range(init.shape[0])]))
    if ev:
        eng.set_evolve_temps(ev); lad.evolve_temps(ev)
    check_name(eng, start)
    PU.assert_same_state(eng, lad, "start")
    done = 0
    while done < steps:
        n = min(10, steps - done)
        eng.step(n); eng.sync(); lad.pt_step(n)
        done += n
        PU.assert_same_state(eng, lad, "after %d steps" % done)
    PU.assert_same_history_and_map(eng, lad, cap)
    if ev:
        assert np.array_equal(eng.invtemps(), lad.betaw)
    assert eng.naccept.sum() - eng.Nc > 10
    eng.close()


def case_lanes(D, Nt, W, ev, aged=False):
    """more than 8 dimensions on a small population: the lanes kernel's propose and accept passes around the device function
    (aged: after the first six steps engine and checker are put late in a run, tests/aging_util.py: the next six cross PT step 2^32)"""
    rng = np.random.default_rng(7)
    c, k = poly_coefs(D, seed=D + 1)
    beta = E.geometric_ladder(Nt, 1e3)
    blo, bhi, bmin, bmax = [0] * D, [0] * D, [0.0] * D, [0.0] * D
    blo[1], bhi[1], bmin[1], bmax[1] = 3, 3, -2.0, 2.0
    types, cen, hw = [1] * D, [0.0] * D, [4.0] * D
    types[2], cen[2], hw[2] = 2, 0.2, 1.5
    x0 = rng.uniform(-1.5, 1.5, size=(Nt * W, D))
    fac = np.tile(np.full(D, 0.4), (Nt, 1)) / np.sqrt(beta)[:, None].clip(1e-2)
    eng = E.Engine(D, Nt, W, swap_rate=0.3)
    eng.set_bounds(blo, bhi, bmin, bmax)
    eng.set_prior(types, cen, hw)
    eng.set_target_device(poly_torch(c, k))
    eng.set_ladder(beta)
    eng.set_proposals(E.PROP_DIAG, fac, np.full(Nt, 0.3))
    eng.set_states(x0)
    check_name(eng, "sweep_lanes_kernel<")
    pb = O.Problem(D)
    pb.set_bounds(blo, bhi, bmin, bmax)
    pb.set_prior(types, cen, hw)
    pb.set_user(poly_numpy(c, k))
    lad = O.Ladder(pb, beta, W=W, swap_rate=0.3)
    lad.set_proposals([(O.PROP_DIAG, fac[r], 0.3) for r in range(Nt)])
    lad.use_philox(0x5EED0001)
    lad.set_states(PU.to_oracle_order(x0, Nt, W))
    if ev:
        eng.set_evolve_temps(ev); lad.evolve_temps(ev)
    PU.assert_same_state(eng, lad, "start")
    view, shift = eng, 0
    for s in range(5):
        eng.step(6); eng.sync(); lad.pt_step(6)
        PU.assert_same_state(view, lad, "after %d steps" % (6 * (s + 1)))
        if aged and s == 0:
            import aging_util as AU
            view, shift = AU.age_pair(eng, lad, 24, step=2**32 - 3)
            check_name(eng, "sweep_lanes_kernel<")
            PU.assert_same_state(view, lad, "aged")
    if aged:
        assert eng.step_count == lad.step == 2**32 - 3 + 24
        assert 2**31 - 2**16 < int(max(eng.ntries.max(), eng.nhist.max())) <= AU.COUNT_MAX - AU.MARGIN
    assert eng.naccept.astype(np.int64).sum() - eng.Nc * (1 + shift) > 5
    eng.close()


def case_general():
    """whole waves per rung at 32 dimensions: the general VALU kernel's passes (no matrix cores on this path)"""
    case_recipe(32, 16, 128, E.PROP_LOWER, 12, 0.0, 0.0, 0, 0, start="sweep_kernel<32,")


# ---------------------------------------------------------------------------------------------------------- device vs host
def _lisa_engine(Nt, W, ev, de, target, seed=0x5EED0001, hist=0):
    D = 6
    beta = E.geometric_ladder(Nt, 1e9)
    sig = np.array(lisa_toy.SCALES) / 20.0
    eng = E.Engine(D, Nt, W, seed=seed, swap_rate=0.3, history_rungs=Nt if hist else 0, history_capacity=hist, map_rungs=Nt if hist else 0)
    eng.set_bounds(lisa_toy.BLO, lisa_toy.BHI, lisa_toy.BMIN, lisa_toy.BMAX)
    eng.set_prior(lisa_toy.TYPES, lisa_toy.CENTERS, lisa_toy.SCALES)
    target(eng)
    eng.set_ladder(beta)
    eng.set_proposals(E.PROP_DIAG, np.tile(sig, (Nt, 1)) / np.sqrt(beta)[:, None].clip(1e-3), np.full(Nt, 0.5))
    if de:
        cum, scales, odfs = _recipe(Nt, 4, 0.8, 0.5)
        eng.set_proposal_mixture(cum, scales, odfs)
        eng.set_proposal_de(0.1, 0.3, 4.0, 0.0)
    if ev:
        eng.set_evolve_temps(ev)
    return eng


def _same(a, b, what):
    for name in ("llike", "lprior", "ntries", "naccept", "last_type", "nhist"):
        u, v = getattr(a, name), getattr(b, name)
        assert np.array_equal(u, v, equal_nan=True), (what, name, np.argwhere(u != v)[:4].tolist())
    assert np.array_equal(a.states(), b.states()), what
    assert np.array_equal(a.invtemps(), b.invtemps()), what


def case_vs_host(Nt, W, ev, de):
    """the same torch toy-LISA function as a device target and wrapped as a host callback: identical chains"""
    hist = 80 if de else 0
    dev = _lisa_engine(Nt, W, ev, de, lambda e: e.set_target_device(lisa_torch), hist=hist)
    host = _lisa_engine(Nt, W, ev, de, lambda e: e.set_target_callback(host_of(lisa_torch, 6), batched=True), hist=hist)
    rng = np.random.default_rng(11)
    lo = np.array(lisa_toy.CENTERS) - np.array(lisa_toy.SCALES)
    hi = np.array(lisa_toy.CENTERS) + np.array(lisa_toy.SCALES)
    x0 = rng.uniform(lo + 0.05, hi - 0.05, size=(Nt * W, 6))
    dev.set_states(x0); host.set_states(x0)
    check_name(dev)
    assert not host.step_kernel_name.endswith(SUFFIX)
    _same(dev, host, "start")
    for s in range(3):
        dev.step(10); host.step(10); dev.sync(); host.sync()
        _same(dev, host, "after %d steps" % (10 * (s + 1)))
    if hist:
        hd, hh = dev.history(), host.history()
        for key in hd:
            assert np.array_equal(hd[key], hh[key], equal_nan=True), key
        md, mh = dev.map(), host.map()
        for key in md:
            assert np.array_equal(md[key], mh[key]), key
    assert dev.naccept.sum() - dev.Nc > 20
    dev.close(); host.close()


# ---------------------------------------------------------------------------------------------------------- set-up
def case_setup():
    """set_states without llike, init_from_prior_k with a likelihood that is -inf on half the prior (redraws), draw_prior_rows:
    the device path equals the host-callback path (and set_states the oracle)"""
    D, Nt, W = 6, 8, 16
    c, k = poly_coefs(D)
    cut = (lisa_toy.CENTERS[0], 1e300)   # -inf for d above the prior's centre: half the prior
    dev = _lisa_engine(Nt, W, 0.0, False, lambda e: e.set_target_device(poly_torch(c, k, cut)))
    host = _lisa_engine(Nt, W, 0.0, False, lambda e: e.set_target_callback(poly_numpy(c, k, cut)))
    for kd in (0, 3):
        dev.init_from_prior(kd); host.init_from_prior(kd)
        _same(dev, host, "init_from_prior(%d)" % kd)
        assert (dev.states()[:, 0] <= cut[0]).all()
    xd, ld, pd = dev.draw_prior_rows(2, 3)
    xh, lh, ph = host.draw_prior_rows(2, 3)
    assert np.array_equal(xd, xh) and np.array_equal(ld, lh) and np.array_equal(pd, ph)
    assert np.isfinite(ld).all()
    # set_states without llike against the oracle
    x0 = dev.states()
    dev.set_states(x0)
    pb = O.Problem(D)
    pb.set_bounds(lisa_toy.BLO, lisa_toy.BHI, lisa_toy.BMIN, lisa_toy.BMAX)
    pb.set_prior(lisa_toy.TYPES, lisa_toy.CENTERS, lisa_toy.SCALES)
    pb.set_user(poly_numpy(c, k, cut))
    lad = O.Ladder(pb, E.geometric_ladder(Nt, 1e9), W=W, swap_rate=0.3)
    lad.use_philox(0x5EED0001)
    lad.set_states(PU.to_oracle_order(x0, Nt, W))
    PU.assert_same_state(dev, lad, "set_states")
    # debug_evaluate returns the device function's llikes
    v, xe, lp, ll = dev.debug_evaluate(x0[:37])
    want = np.array([poly_numpy(c, k, cut)(r) for r in xe])
    assert np.array_equal(ll, want)
    dev.close(); host.close()


# ---------------------------------------------------------------------------------------------------------- best posterior
def case_best(Nt, W, ev):
    """best_evaluated() is the maximum of lprior + llike over every row the function was asked to evaluate (ties: the first)"""
    D = 6
    c, k = poly_coefs(D)
    k = [v * 40.0 for v in k]
    rec = {"on": True, "b": []}
    tf = poly_torch(c, k)

    def fn(X, count, out):
        tf(X, count, out)
        if rec["on"]:
            rec["b"].append((X.clone(), count.clone(), out.clone()))
    eng = _lisa_engine(Nt, W, ev, True, lambda e: e.set_target_device(fn), hist=64)
    lp0, x0b = eng.best_evaluated()
    assert lp0 == -math.inf and not x0b.any()
    rec["b"].clear()
    eng.init_from_prior()
    eng.step(25)
    eng.sync()
    rec["on"] = False
    best_v, best_x = -math.inf, None
    for X, cnt, out in rec["b"]:
        n = int(cnt.item())
        assert X.shape[0] == eng.Nc
        if n == 0:
            continue
        Xn = X[:n].cpu().numpy()
        lp = eng.debug_evaluate(Xn)[2]
        post = lp + out[:n].cpu().numpy()
        j = int(np.nanargmax(np.where(np.isnan(post), -np.inf, post)))
        if post[j] > best_v:
            best_v, best_x = post[j], Xn[j]
    got_v, got_x = eng.best_evaluated()
    assert got_v == best_v, (got_v, best_v)
    assert np.array_equal(got_x, best_x)
    eng.set_states(eng.states())   # a state set-up starts over (and evaluates the states it sets)
    v2, _ = eng.best_evaluated()
    assert v2 == np.max(eng.lprior + eng.llike)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- contract
def case_contract():
    D, Nt, W = 6, 20, 64
    calls = {"n": 0, "rows": set()}
    tf = poly_torch(*poly_coefs(D))

    def fn(X, count, out):
        calls["n"] += 1
        calls["rows"].add(X.shape[0])
        tf(X, count, out)
    eng = _lisa_engine(Nt, W, 0.01, True, lambda e: e.set_target_device(fn), hist=256)
    assert eng.target_device_rows == Nt * W
    eng.init_from_prior()
    eng.sync()
    calls["n"] = 0
    eng.step(200)   # queued: the function has run 200 times (once per sweep) before anything waited
    assert calls["n"] == 200, calls
    eng.sync()
    assert calls["rows"] == {Nt * W}, calls
    # refusals: prior callback, host-side proposals, partial sweeps / exchange phases, rung shards
    for bad in (lambda: eng.set_prior_callback(lambda x: 0.0),
                lambda: eng.sweep_rungs(0, 1, False),
                lambda: eng.exchange_decide(None, None, 0, None, None)):
        try:
            bad()
        except E.PtmError as ex:
            assert "ptm error -2" in str(ex), ex
        else:
            raise AssertionError("not refused")
    shard = E.Engine(D, Nt, W, rung_begin=0, rung_count=Nt // 2)
    try:
        shard.set_target_device(fn)
    except E.PtmError as ex:
        assert "ptm error -2" in str(ex), ex
    else:
        raise AssertionError("a rung shard took a device likelihood")
    shard.close()
    # the last target setter wins
    check_name(eng)
    eng.set_target_callback(poly_numpy(*poly_coefs(D)))
    assert not eng.step_kernel_name.endswith(SUFFIX)
    eng.set_target_device(fn)
    check_name(eng)
    P = np.eye(D)
    eng.set_target_gaussian(P, 0.0)
    assert not eng.step_kernel_name.endswith(SUFFIX)
    n0 = calls["n"]
    eng.step(3); eng.sync()
    assert calls["n"] == n0
    eng.close()
    # walkers split: an ordinary engine on walkers [W/2, W) takes it and matches the whole engine's upper walkers' start
    half = E.Engine(D, Nt, W // 2, walker_begin=W // 2)
    half.set_bounds(lisa_toy.BLO, lisa_toy.BHI, lisa_toy.BMIN, lisa_toy.BMAX)
    half.set_prior(lisa_toy.TYPES, lisa_toy.CENTERS, lisa_toy.SCALES)
    half.set_target_device(tf)
    assert half.target_device_rows == Nt * W // 2
    half.close()


# ---------------------------------------------------------------------------------------------------------- the HIP example
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ROOT = os.path.dirname(HERE)


def _build_example(d):
    so = os.path.join(d, "liblisa_device.so")
    import subprocess
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "lisa_device_likelihood.hip"), "-o", so])
    import ctypes as C
    lib = C.CDLL(so)
    return lib, C.cast(lib.lisa_loglike_device, C.c_void_p).value


def _prior_draws(n, seed=5):
    rng = np.random.default_rng(seed)
    lo = np.array(lisa_toy.CENTERS) - np.array(lisa_toy.SCALES)
    hi = np.array(lisa_toy.CENTERS) + np.array(lisa_toy.SCALES)
    return rng.uniform(lo, hi, size=(n, 6))


def _launcher_torch(lib):
    """the example's launcher as a torch-style function (for the host round trip): X, count, out on the current stream"""
    import ctypes as C
    f = lib.lisa_loglike_device
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    def g(X, count, out):
        f(None, C.c_void_p(torch.cuda.current_stream().cuda_stream), X.shape[0], X.shape[1], C.c_void_p(X.data_ptr()),
          C.c_void_p(count.data_ptr()), C.c_void_p(out.data_ptr()))
    return g


def case_hip_example():
    import tempfile
    import subprocess
    with tempfile.TemporaryDirectory() as d:
        lib, fp = _build_example(d)
        g = _launcher_torch(lib)
        # 1. its llikes against lisa_toy.loglike on 10^4 in-prior states
        X = _prior_draws(10000)
        Xt = torch.as_tensor(X, device=DEV)
        out = torch.empty(X.shape[0], dtype=torch.float64, device=DEV)
        g(Xt, torch.full((1,), X.shape[0], dtype=torch.int32, device=DEV), out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want = np.array([lisa_toy.loglike(x) for x in X])
        rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
        assert rel.max() < 1e-12, rel.max()
        # 2. an engine driven by it (set_target_device_c) against one whose host callback round-trips the same launcher
        Nt, W = 20, 4
        dev = _lisa_engine(Nt, W, 0.01, True, lambda e: e.set_target_device_c(fp), hist=64)
        host = _lisa_engine(Nt, W, 0.01, True, lambda e: e.set_target_callback(host_of(g, 6), batched=True), hist=64)
        x0 = _prior_draws(Nt * W, seed=9)
        dev.set_states(x0); host.set_states(x0)
        check_name(dev)
        _same(dev, host, "start")
        for s in range(3):
            dev.step(10); host.step(10); dev.sync(); host.sync()
            _same(dev, host, "after %d steps" % (10 * (s + 1)))
        dev.close(); host.close()
        # 3. example_lisa_device: the device and the host path write the same chain files
        exe = os.path.join(d, "lisa_device")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), os.path.join(ROOT, "examples", "example_lisa_device.cc"),
                               os.path.join(ROOT, "examples", "lisa_device_likelihood.hip"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
                               "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-o", exe])
        best = {}
        for mode in ("1", "0"):
            env = dict(os.environ, PTM_DEVICE_LIKE=mode)
            env.pop("PTM_HOST_DE", None)
            r = subprocess.run([exe, "--outname=run" + mode, "--pt=8", "--replicas=4", "--nsteps=600", "--nevery=200", "--seed=0.4"],
                               capture_output=True, text=True, timeout=600, cwd=d, env=env)
            assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
            line = [l for l in r.stdout.splitlines() if l.startswith("best_post ")][-1]
            best[mode] = float(line.split()[1].rstrip(","))
        files = sorted(f for f in os.listdir(d) if f.startswith("run1") and f.endswith(".dat"))
        assert files, os.listdir(d)
        for f in files:
            a = open(os.path.join(d, f), "rb").read()
            b = open(os.path.join(d, "run0" + f[4:]), "rb").read()
            assert a == b, f
        assert abs(best["1"] - best["0"]) <= 1e-9 * abs(best["0"]), best


CASES = {"c5": case_c5, "recipe": case_recipe, "lanes": case_lanes, "general": case_general, "vs_host": case_vs_host,
         "setup": case_setup, "best": case_best, "contract": case_contract,
         "hip_example": case_hip_example}

if __name__ == "__main__":
    torch.cuda.init()
    name, args = sys.argv[1], json.loads(sys.argv[2]) if len(sys.argv) > 2 else []
    CASES[name](*args)
    print("OK", name, args, flush=True)
