"""Child process of tests/test_gpu_device_prior.py: user priors written in torch, run by the engine ON THE DEVICE
(ptm_set_prior_device) beside a device likelihood, against the CPU oracle and against the host-callback path.

torch is imported FIRST (tests/torch_shard_worker.py says why: one HIP runtime per process).  Usage: device_prior_worker.py CASE [ARGS..];
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
from device_like_worker import DEV, SUFFIX, _lisa_engine, _prior_draws, _same, host_of, lisa_torch, poly_coefs, poly_numpy, poly_torch
from ptmcmc_amd import engine as E

SEED = 0x5EED0001
NAME = " + device prior + device likelihood"
assert NAME.endswith(SUFFIX)


# -- the prior of test_host_evaluated_prior_matches_the_oracle (a correlated Gaussian times a hard disc in the first two dimensions)
#    in a form whose torch and numpy bits agree: + - * only, one elementwise op per kernel, the columns summed in index order
def disc_prior_numpy(D, seen=None):
    def f(x):
        x0, x1 = float(x[0]), float(x[1])
        if seen is not None:
            seen.append(np.array(x, dtype=np.float64))
        r2 = x0 * x0
        r2 = r2 + x1 * x1
        if r2 > 6.0:
            return -math.inf
        t = x0 - 0.3 * x1
        t = t * t
        t = t * (-0.5)
        s = 0.0
        for d in range(2, D):
            u = float(x[d])
            s = s + u * u
        t = t - 0.05 * s
        return t - 1.234
    return f


def disc_prior_torch(D):
    def f(X, count, out):
        x0, x1 = X[:, 0], X[:, 1]
        r2 = x0 * x0
        r2 = r2 + x1 * x1
        t = x0 - 0.3 * x1
        t = t * t
        t = t * (-0.5)
        s = torch.zeros(X.shape[0], dtype=torch.float64, device=X.device)
        for d in range(2, D):
            u = X[:, d]
            s = s + u * u
        t = t - 0.05 * s
        t = t - 1.234
        out.copy_(torch.where(r2 > 6.0, torch.full_like(t, -math.inf), t))
    return f


def recorder(fn, rec):
    def g(X, count, out):
        fn(X, count, out)
        if rec["on"]:
            rec["b"].append((X.clone(), count.clone(), out.clone()))
    return g


def _rows(rec):
    """the recorded calls on the host: (rows below the count, their outputs, n_rows)"""
    return [(X[:int(c.item())].cpu().numpy(), o[:int(c.item())].cpu().numpy(), X.shape[0]) for X, c, o in rec["b"]]


def disc_setup(D, Nt, W, ev, sigma=0.6, odf=0.2, bounds=None, x0=None, hist=0):
    """engine (device prior + device likelihood, both recorded) and checker of the disc-prior problem at the same start states"""
    rng = np.random.default_rng(11)
    c, k = poly_coefs(D, seed=D)
    beta = E.geometric_ladder(Nt, 1e3)
    if bounds is None:
        blo, bhi, bmin, bmax = [0] * D, [0] * D, [0.0] * D, [0.0] * D
        blo[1], bhi[1], bmin[1], bmax[1] = 3, 3, -2.0, 2.0                     # wrap
        blo[2], bhi[2], bmin[2], bmax[2] = 1, 1, -3.0, 3.0                     # limit: proposals beyond it are invalid
        bounds = (blo, bhi, bmin, bmax)
    if x0 is None:
        x0 = rng.uniform(-1.2, 1.2, size=(Nt * W, D))
    fac = np.tile(np.full(D, sigma), (Nt, 1)) / np.sqrt(beta)[:, None].clip(1e-2)
    prec, lrec = {"on": True, "b": []}, {"on": True, "b": []}
    eng = E.Engine(D, Nt, W, seed=SEED, swap_rate=0.3, history_rungs=Nt if hist else 0, history_capacity=hist, map_rungs=Nt if hist else 0)
    eng.set_bounds(*bounds)
    eng.set_target_device(recorder(poly_torch(c, k), lrec))
    eng.set_prior_device(recorder(disc_prior_torch(D), prec))
    eng.set_ladder(beta)
    eng.set_proposals(E.PROP_DIAG, fac, np.full(Nt, odf))
    eng.set_states(x0)
    seen = []
    pb = O.Problem(D)
    pb.set_bounds(*bounds)
    pb.set_user(poly_numpy(c, k))
    pb.set_user_prior(disc_prior_numpy(D, seen))
    lad = O.Ladder(pb, beta, W=W, swap_rate=0.3)
    lad.set_proposals([(O.PROP_DIAG, fac[r], odf) for r in range(Nt)])
    lad.use_philox(SEED)
    if hist:
        lad.enable_history(hist)
    lad.set_states(PU.to_oracle_order(x0, Nt, W))
    if ev:
        eng.set_evolve_temps(ev); lad.evolve_temps(ev)
    return eng, lad, prec, lrec, seen, x0


def check_name(eng, start=None):
    nm = eng.step_kernel_name
    assert nm.endswith(NAME) and nm.startswith("decide_kernel + "), nm
    if start:
        assert eng.sweep_kernel_name.startswith(start), eng.sweep_kernel_name


# ---------------------------------------------------------------------------------------------------------- 1. oracle parity
def case_oracle(D, Nt, W, ev):
    eng, lad, prec, lrec, seen, x0 = disc_setup(D, Nt, W, ev)
    check_name(eng, "sweep_kernel<32," if W % 64 == 0 else "sweep_lanes_kernel<")
    PU.assert_same_state(eng, lad, "start")
    for s in range(6):
        eng.step(5); eng.sync(); lad.pt_step(5)
        PU.assert_same_state(eng, lad, "after %d steps" % (5 * (s + 1)))
        if ev:
            assert np.array_equal(eng.invtemps(), lad.betaw)
    prec["on"] = lrec["on"] = False
    pr, lr = _rows(prec), _rows(lrec)
    assert len(pr) == len(lr) == 31, (len(pr), len(lr))        # the set-up call and one call per step, each
    out_disc = 0
    for X, o, n in pr:
        assert n == Nt * W
        assert (np.abs(X[:, 1]) <= 2.0).all() and (np.abs(X[:, 2]) <= 3.0).all()      # never a state outside the boundaries
        out_disc += int((X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1] > 6.0).sum())
    for X, o, n in lr:
        assert n == Nt * W
        assert not (X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1] > 6.0).any()                 # never a state outside the prior's support
    assert out_disc > 0          # (a condition on the inputs: the checker's own prior calls say the same, below)
    so = np.array(seen)
    assert (so[:, 0] * so[:, 0] + so[:, 1] * so[:, 1] > 6.0).sum() >= out_disc > 0
    lp = eng.lprior
    assert np.isfinite(lp).all() and len(np.unique(lp)) > Nt * W // 2
    assert eng.naccept.sum() - eng.Nc > 10
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 2. empty batches
def case_empty():
    D, Nt, W = 3, 6, 4
    bounds = ([1] * D, [1] * D, [-0.5] * D, [0.5] * D)
    x0 = np.random.default_rng(3).uniform(-0.4, 0.4, size=(Nt * W, D))
    eng, lad, prec, lrec, seen, x0 = disc_setup(D, Nt, W, 0.0, sigma=1e6, odf=0.0, bounds=bounds, x0=x0)
    check_name(eng)
    PU.assert_same_state(eng, lad, "start")
    prec["b"].clear(); lrec["b"].clear()
    for s in range(3):
        eng.step(10); eng.sync(); lad.pt_step(10)
        PU.assert_same_state(eng, lad, "after %d steps" % (10 * (s + 1)))
    prec["on"] = lrec["on"] = False
    assert len(prec["b"]) == len(lrec["b"]) == 30
    for rec in (prec, lrec):
        for X, cnt, out in rec["b"]:
            assert int(cnt.item()) == 0 and X.shape[0] == Nt * W
    moved = np.sort(eng.states(), axis=0) != np.sort(x0, axis=0)      # (exchanges permute a ladder's states; nothing new appears)
    assert not moved.any()
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 3. device vs host
def trans_prior_torch(X, count, out):
    """transcendental functions: the same on both paths only because both paths run THIS function on the device"""
    d, inc = X[:, 0], X[:, 2]
    u, v = d - 1.7, inc - 1.5
    r = -0.5 * (u * u + 0.6 * u * v + v * v) + 0.3 * torch.cos(inc) * u - torch.exp(-d)
    out.copy_(torch.where(d > 2.8, torch.full_like(r, -math.inf), r))


def _start(n, seed):
    """start states inside the toy-LISA box and inside trans_prior_torch's support"""
    x0 = _prior_draws(n, seed=seed) * 0.9 + 0.1 * np.array(lisa_toy.CENTERS)
    x0[:, 0] = np.minimum(x0[:, 0], 2.7)
    return x0


def case_vs_host(Nt, W, ev, de):
    hist = 80 if de else 0

    def dev_side(e):
        e.set_prior_device(trans_prior_torch)      # (before the target: the setters come in either order)
        e.set_target_device(lisa_torch)

    def host_side(e):
        e.set_target_callback(host_of(lisa_torch, 6), batched=True)
        e.set_prior_callback(host_of(trans_prior_torch, 6), batched=True)
    dev = _lisa_engine(Nt, W, ev, de, dev_side, hist=hist)
    host = _lisa_engine(Nt, W, ev, de, host_side, hist=hist)
    x0 = _start(Nt * W, seed=11)
    dev.set_states(x0); host.set_states(x0)
    check_name(dev)
    assert "device" not in host.step_kernel_name
    _same(dev, host, "start")
    assert len(np.unique(dev.lprior)) > Nt * W // 2
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


# ------------------------------------------------------------------------------------------------- 4. beside device proposals
def case_devprop(D, Nt, W):
    """the scripted proposal of tests/test_gpu_device_proposals.py (the HIP launcher; the checker: its numpy twin) with a device prior
    and a device likelihood: the whole step on the device, against the oracle"""
    import tempfile

    import test_gpu_device_proposals as T
    from ptmcmc_amd.problems import GaussianProblem
    from test_gpu_host_proposals import scripted_proposal
    c, k = poly_coefs(D, seed=D)
    with tempfile.TemporaryDirectory() as d:
        lib = T.build_example(d)
        pr = GaussianProblem(D, Nt, 1e3)
        scale = T.scale_for(pr, D)
        x0 = np.random.default_rng(5).uniform(-1.0, 1.0, size=(Nt * W, D)) * np.sqrt(np.diag(pr.cov))
        x0[:, :2] *= 1.5 / max(1.5, np.abs(x0[:, :2]).max())      # inside the disc
        eng = E.Engine(D, Nt, W, seed=T.SEED, swap_rate=0.35)
        pr.configure(eng, E.PROP_DIAG)
        la = T.Launcher(lib, scale, Nt * W)
        la.attach(eng)
        eng.set_target_device(poly_torch(c, k))
        eng.set_prior_device(disc_prior_torch(D))
        eng.set_states(x0)
        check_name(eng, "sweep_lanes_kernel<")
        pb = PU.oracle_problem(pr)
        pb.set_user(poly_numpy(c, k))
        pb.set_user_prior(disc_prior_numpy(D))
        lad = O.Ladder(pb, pr.beta, W=W, swap_rate=0.35)
        lad.set_proposals([(O.PROP_DIAG, np.ones(D), 0.0)] * Nt)
        lad.use_philox(T.SEED)
        lad.set_host_proposal(O.make_propose_fn(scripted_proposal(scale)))
        lad.set_states(PU.to_oracle_order(x0, Nt, W))
        PU.assert_same_state(eng, lad, "start")
        for s in range(6):
            eng.step(5); eng.sync(); lad.pt_step(5)
            PU.assert_same_state(eng, lad, "after %d steps" % (5 * (s + 1)))
            T.check_outcome(eng, lad, la)
        assert la.user.calls == 30
        acc, tries = int(eng.naccept.sum()) - eng.Nc, int(eng.ntries.sum()) - eng.Nc
        assert 0 < acc < tries, (acc, tries)
        eng.close()


# ---------------------------------------------------------------------------------------------------------- 5. set-up and best
def case_setup_best():
    D, Nt, W = 6, 8, 5
    eng, lad, prec, lrec, seen, x0 = disc_setup(D, Nt, W, 0.0)
    PU.assert_same_state(eng, lad, "set_states without llike")
    pn = disc_prior_numpy(D)
    # debug_evaluate: the function's log-priors for the valid rows, -inf for a row a `limit` bound makes invalid
    prec["on"] = lrec["on"] = False
    Xq = np.concatenate([x0[:37], [[0.1] * 2 + [3.5] + [0.0] * (D - 3)], [[2.4, 1.0] + [0.0] * (D - 2)]])
    v, xe, lp, ll = eng.debug_evaluate(Xq)
    want = np.array([pn(r) if ok else -math.inf for r, ok in zip(xe, v)])
    assert np.array_equal(lp, want), (lp, want)
    assert v[-2] == 0 and lp[-2] == -math.inf and v[-1] != 0 and lp[-1] == -math.inf and np.isfinite(lp[:37]).all()
    prec["on"] = lrec["on"] = True
    # the kept best: lprior + llike over the rows the likelihood was asked about, with the prior's recorded values for those rows
    eng.step(25); eng.sync()
    prec["on"] = lrec["on"] = False
    pr, lr = _rows(prec), _rows(lrec)
    assert len(pr) == len(lr) == 26
    best_v, best_x = -math.inf, None
    for (Xp, op, _), (Xl, ol, _) in zip(pr, lr):
        lp_of = {r.tobytes(): val for r, val in zip(Xp, op)}
        for r, llv in zip(Xl, ol):
            post = lp_of[r.tobytes()] + llv      # (every row the likelihood saw, the prior saw in the same call pair)
            if post > best_v:
                best_v, best_x = post, r
    got_v, got_x = eng.best_evaluated()
    assert got_v == best_v, (got_v, best_v)
    assert np.array_equal(got_x, best_x)
    eng.set_states(eng.states())      # a state set-up starts over, from the user's lprior
    v2, _ = eng.best_evaluated()
    assert v2 == np.max(eng.lprior + eng.llike)
    # a checkpoint goes back through ptm_restore: the same lpriors, from the function
    ck = eng.checkpoint()
    lp0 = eng.lprior.copy()
    eng.restore(ck)
    assert np.array_equal(eng.lprior, lp0)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 6. contract
def _refused(what, fn):
    try:
        fn()
    except E.PtmError as ex:
        assert "ptm error -2" in str(ex), (what, ex)
    else:
        raise AssertionError("not refused: " + what)


def case_contract():
    D, Nt, W = 6, 20, 64
    calls = {"p": 0, "l": 0, "rows": set()}
    tl = poly_torch(*poly_coefs(D))

    def prior(X, count, out):
        calls["p"] += 1
        calls["rows"].add(X.shape[0])
        trans_prior_torch(X, count, out)

    def like(X, count, out):
        calls["l"] += 1
        calls["rows"].add(X.shape[0])
        tl(X, count, out)
    x0 = _start(Nt * W, seed=9)

    def both(e):
        e.set_target_device(like); e.set_prior_device(prior)
    eng = _lisa_engine(Nt, W, 0.01, True, both, hist=256)
    assert eng.target_device_rows == Nt * W
    eng.set_states(x0)
    eng.sync()
    calls["p"] = calls["l"] = 0
    eng.step(200)      # queued: both functions have run 200 times (once per sweep) before anything waited
    assert calls["p"] == 200 and calls["l"] == 200, calls
    eng.sync()
    assert calls["rows"] == {Nt * W}, calls
    # refusals, each -2, and the engine goes on stepping
    _refused("prior callback beside a device prior", lambda: eng.set_prior_callback(lambda x: 0.0))
    _refused("host-side proposals", lambda: eng.set_proposal_callback(lambda X, r, w, s: (X, np.zeros(len(X)), np.zeros(len(X), np.int32), np.ones(len(X), np.int32))))
    _refused("partial sweep", lambda: eng.sweep_rungs(0, 1, False))
    _refused("exchange phase", lambda: eng.exchange_decide(None, None, 0, None, None))
    _refused("init_from_prior", lambda: eng.init_from_prior())
    _refused("init_from_prior_k", lambda: eng.init_from_prior(2))
    _refused("draw_prior_rows", lambda: eng.draw_prior_rows(1, 2))
    _refused("prior draw member", lambda: eng.set_proposal_prior_draw(1))
    check_name(eng)
    n0 = calls["p"]
    eng.step(3); eng.sync()
    assert calls["p"] == n0 + 3 and calls["l"] == n0 + 3
    ref = [getattr(eng, a).copy() for a in ("llike", "lprior", "ntries", "naccept")] + [eng.states()]
    # without the device likelihood: refused at set_states, restore and step; the states stay as they were
    ck = eng.checkpoint()
    eng.set_target_callback(poly_numpy(*poly_coefs(D)))
    _refused("step without the device likelihood", lambda: eng.step(1))
    _refused("set_states without the device likelihood", lambda: eng.set_states(x0))
    _refused("restore without the device likelihood", lambda: eng.restore(ck))
    P = np.eye(D)
    eng.set_target_gaussian(P, 0.0)
    _refused("step beside the built-in Gaussian target", lambda: eng.step(1))
    eng.set_target_device(like)
    for a, b in zip(ref, [getattr(eng, a) for a in ("llike", "lprior", "ntries", "naccept")] + [eng.states()]):
        assert np.array_equal(a, b)
    eng.step(2); eng.sync()
    assert calls["p"] == n0 + 5
    eng.close()
    # a rung shard refuses; a host prior refuses a device prior after it
    shard = E.Engine(D, Nt, W, rung_begin=0, rung_count=Nt // 2)
    _refused("rung shard", lambda: shard.set_prior_device(prior))
    shard.close()
    hp = _lisa_engine(4, 2, 0.0, False, lambda e: (e.set_target_callback(poly_numpy(*poly_coefs(D))), e.set_prior_callback(lambda x: 0.0)))
    _refused("device prior beside a prior callback", lambda: hp.set_prior_device(prior))
    hp.set_states(x0[:8]); hp.step(2); hp.sync()
    hp.close()
    # set_prior_device(None): back to the built-in prior -- the chain of an engine that never had one; and the setters' order is free
    Nt2, W2 = 8, 4
    x1 = x0[:Nt2 * W2]
    a = _lisa_engine(Nt2, W2, 0.0, False, lambda e: (e.set_prior_device(trans_prior_torch), e.set_target_device(tl)))
    b = _lisa_engine(Nt2, W2, 0.0, False, lambda e: (e.set_target_device(tl), e.set_prior_device(trans_prior_torch)))
    never = _lisa_engine(Nt2, W2, 0.0, False, lambda e: e.set_target_device(tl))
    a.set_states(x1); b.set_states(x1)
    a.step(12); b.step(12); a.sync(); b.sync()
    _same(a, b, "prior before / after the target")
    assert a.naccept.sum() - a.Nc > 5
    a.set_prior_device(None)
    assert a.step_kernel_name.endswith(SUFFIX) and not a.step_kernel_name.endswith(NAME)
    a.set_states(x1); never.set_states(x1)
    a.step(12); never.step(12); a.sync(); never.sync()
    _same(a, never, "after set_prior_device(None)")
    assert not np.array_equal(a.states(), b.states())
    a.close(); b.close(); never.close()


# ---------------------------------------------------------------------------------------------------------- 7. the HIP example
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ROOT = os.path.dirname(HERE)


def case_hip_example():
    import ctypes as C
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        ex = os.path.join(ROOT, "examples")
        inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), "-I", ex]
        so = os.path.join(d, "libcorrelated_prior.so")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-ffp-contract=off"] + inc +
                              [os.path.join(ex, "correlated_prior_device.hip"), "-o", so])
        lib = C.CDLL(so)
        # 1. the kernel against the host form (the same inline function, compiled for the host) on 10^4 in-prior states: equal bits
        X = _prior_draws(10000)
        Xt = torch.as_tensor(X, device=DEV)
        out = torch.empty(X.shape[0], dtype=torch.float64, device=DEV)
        f = lib.correlated_logprior_device
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        f(None, C.c_void_p(torch.cuda.current_stream().cuda_stream), X.shape[0], 6, C.c_void_p(Xt.data_ptr()), None, C.c_void_p(out.data_ptr()))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        h = lib.correlated_logprior_host
        h.argtypes = [C.POINTER(C.c_double)]
        h.restype = C.c_double
        want = np.array([h(np.ascontiguousarray(x).ctypes.data_as(C.POINTER(C.c_double))) for x in X])
        assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
        assert np.isfinite(want).sum() > 1000 and np.isinf(want).sum() > 100      # both sides of the hard cut
        # 2. example_lisa_device_prior: the device and the host route write the same chain files
        exe = os.path.join(d, "lisa_device_prior")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off"] + inc +
                              [os.path.join(ex, "example_lisa_device_prior.cc"), os.path.join(ex, "lisa_device_likelihood.hip"),
                               os.path.join(ex, "correlated_prior_device.hip"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
                               "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-o", exe])
        outs = {}
        for mode in ("1", "0"):
            env = dict(os.environ, PTM_DEVICE_PRIOR=mode)
            env.pop("PTM_HOST_DE", None); env.pop("PTM_DEVICE_LIKE", None)
            r = subprocess.run([exe, "--outname=run" + mode, "--pt=8", "--replicas=4", "--nsteps=600", "--nevery=200", "--seed=0.4"],
                               capture_output=True, text=True, timeout=600, cwd=d, env=env)
            assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
            outs[mode] = r.stdout
        files = sorted(f for f in os.listdir(d) if f.startswith("run1") and f.endswith(".dat"))
        assert files, os.listdir(d)
        for fn in files:
            a = open(os.path.join(d, fn), "rb").read()
            b = open(os.path.join(d, "run0" + fn[4:]), "rb").read()
            assert a == b and len(a) > 1000, fn
        k1 = [l for l in outs["1"].splitlines() if l.startswith("step kernel: ")]
        k0 = [l for l in outs["0"].splitlines() if l.startswith("step kernel: ")]
        assert k1 and all(l.endswith(NAME) for l in k1), k1
        assert k0 and not any("device prior" in l for l in k0), k0


CASES = {"oracle": case_oracle, "empty": case_empty, "vs_host": case_vs_host, "devprop": case_devprop, "setup_best": case_setup_best,
         "contract": case_contract, "hip_example": case_hip_example}

if __name__ == "__main__":
    torch.cuda.init()
    name, args = sys.argv[1], json.loads(sys.argv[2]) if len(sys.argv) > 2 else []
    CASES[name](*args)
    print("OK", name, args, flush=True)
