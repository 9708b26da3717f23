"""User proposals drawn ON THE DEVICE (ptm_set_proposal_device): the engine packs the chains that move, calls the user's batched
function on its own stream, unpacks what it wrote and sweeps with ready-made proposals -- no host wait anywhere.

The engine is driven by the HIP launcher of examples/scripted_device_proposal.hip, the device twin of scripted_proposal
(tests/test_gpu_host_proposals.py): the checker is handed the numpy form through set_host_proposal, and both must walk the same
chains bit for bit.  The torch cases run in a child process (tests/device_proposal_worker.py: torch before the engine library)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import parity_util as PU
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem
from test_gpu_host_proposals import scripted_proposal

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SEED = 0x5EED0001


class ScriptedUser(C.Structure):
    """scripted_proposal_user of examples/scripted_device_proposal.hip"""
    _fields_ = [("scale_dev", C.c_void_p), ("accepted_out_dev", C.c_void_p), ("rung_out_dev", C.c_void_p), ("walker_out_dev", C.c_void_p),
                ("count_out_dev", C.c_void_p), ("calls", C.c_uint64), ("result_calls", C.c_uint64), ("last_step", C.c_uint64 * 4)]


def build_example(d):
    so = os.path.join(d, "libscripted_proposal.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "scripted_device_proposal.hip"), "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    return build_example(str(tmp_path_factory.mktemp("devprop")))


class Launcher:
    """the example's launchers with their `user` block: per-rung scales on the device, buffers the result launcher copies into"""

    def __init__(self, lib, scale, n_rows):
        scale = np.ascontiguousarray(scale, dtype=np.float64)
        self.scale = E.DeviceBuffer(scale.nbytes)
        self.scale.copy_from(scale.ctypes.data)
        self.acc, self.rung, self.walker, self.count = (E.DeviceBuffer(4 * max(n_rows, 1)) for _ in range(4))
        fill = np.full(max(n_rows, 1), -7, dtype=np.int32)
        for b in (self.acc, self.rung, self.walker, self.count):
            b.copy_from(fill.ctypes.data)
        self.user = ScriptedUser(self.scale.ptr, self.acc.ptr, self.rung.ptr, self.walker.ptr, self.count.ptr, 0, 0)
        self.propose = C.cast(lib.scripted_propose_device, C.c_void_p).value
        self.result = C.cast(lib.scripted_result_device, C.c_void_p).value

    def attach(self, eng):
        eng.set_proposal_device_c(self.propose, self.result, user=C.addressof(self.user))

    def outcome(self):
        """(count, rung[:count], walker[:count], accepted[:count]) of the last result call; after eng.sync()"""
        n = int(self.count.to_numpy(np.int32)[0])
        return n, self.rung.to_numpy(np.int32)[:n], self.walker.to_numpy(np.int32)[:n], self.acc.to_numpy(np.int32)[:n]


def dp_of(D):
    return 4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else 32 if D <= 32 else 64 if D <= 64 else 128


def scale_for(pr, D):
    return 2.0 / np.sqrt(D) / np.sqrt(np.maximum(pr.beta, 0.02)) * np.sqrt(np.diag(pr.cov).mean())


def general_space(D):
    blo, bhi, bmin, bmax = [0] * D, [0] * D, [0.0] * D, [0.0] * D
    blo[0], bhi[0], bmin[0], bmax[0] = 3, 3, -3.0, 2.5                    # wrap
    blo[1], bhi[1], bmin[1], bmax[1] = 2, 2, -4.0, 4.0                    # reflect
    blo[2], bhi[2], bmin[2], bmax[2] = 1, 1, -6.0, 6.0                    # limit
    types, cen, hw = [1] * D, [0.0] * D, [8.0] * D
    types[1], cen[1], hw[1] = 2, 0.1, 2.0                                  # gaussian
    return (blo, bhi, bmin, bmax), (types, cen, hw), np.linspace(-0.3, 0.3, D)


def diag_loglike(D):
    """the diagonal quadratic of test_gpu_host_proposals: the same bits from the engine's host callback and the checker"""
    sc = np.linspace(0.7, 1.4, D)
    return lambda x: float(-0.5 * np.sum((np.asarray(x) * sc) ** 2))


def host_logprior(x):
    """a prior ptm_set_prior cannot describe: correlated in the first two dimensions, a hard box around it"""
    x = np.asarray(x, dtype=np.float64)
    if np.max(np.abs(x)) > 60.0:
        return -np.inf
    return float(-0.5 * (x[0] - 0.3 * x[1]) ** 2 - 0.05 * np.sum(x[2:] ** 2) - 1.234)


def make_pair(example, D, Nt, W, general=False, cb=False, prior_cb=False, ev=0.0, N=1, sr=0.35, cap=96, seed=SEED):
    """an engine on the HIP launcher and its checker twin on the numpy scripted_proposal, at the same start states"""
    pr = GaussianProblem(D, Nt, 1e3)
    bounds = prior = mean = None
    if general:
        bounds, prior, mean = general_space(D)
    scale = scale_for(pr, D)
    eng = E.Engine(D, Nt, W, seed=seed, swap_rate=sr, add_every_n=N, history_rungs=Nt if cap else 0, history_capacity=cap, map_rungs=Nt if cap else 0)
    pr.configure(eng, E.PROP_DIAG)      # (the engine's own proposals set first: the device function must replace them)
    if bounds: eng.set_bounds(*bounds)
    if prior: eng.set_prior(*prior)
    if mean is not None: eng.set_target_gaussian(pr.P, pr.like0, mean)
    pb = PU.oracle_problem(pr, bounds, prior, mean)
    if cb or prior_cb:
        ll = diag_loglike(D)
        eng.set_target_callback(ll)
        pb.set_user(ll)
    if prior_cb:
        eng.set_prior_callback(host_logprior)
        pb.set_user_prior(host_logprior)
    la = Launcher(example, scale, Nt * W)
    la.attach(eng)
    rng = np.random.default_rng(5)
    x0 = rng.uniform(-1.0, 1.0, size=(Nt * W, D)) * np.sqrt(np.diag(pr.cov))
    eng.set_states(x0)
    cfn = O.make_propose_fn(scripted_proposal(scale))
    lad = O.Ladder(pb, pr.beta, W=W, swap_rate=sr, add_every_N=N)
    lad.set_proposals([(O.PROP_DIAG, np.ones(D), 0.0)] * Nt)       # unused
    lad.use_philox(seed)
    if cap:
        lad.enable_history(cap)
    lad.set_host_proposal(cfn)
    lad.set_states(PU.to_oracle_order(x0, Nt, W))
    if ev:
        eng.set_evolve_temps(ev); lad.evolve_temps(ev)
    return pr, eng, lad, la


def check_outcome(eng, lad, la):
    """the result launcher's copy against the checker: its rows are exactly the moving chains, in order, with their outcomes"""
    Nt, W = eng.Nt, eng.W
    want = PU.to_engine_order(lad.last_accept_mh, Nt, W)
    moving = np.flatnonzero(want != 2)
    n, r, w, a = la.outcome()
    assert n == len(moving), (n, len(moving))
    assert np.array_equal(r.astype(np.int64) * W + w, moving)
    assert np.array_equal(a, want[moving])
    return n


# ---------------------------------------------------------------------------------------------------------------- 1. bit-exact
CASES = [
    # D, Nt, W, general state space, host-callback likelihood, host prior callback, evolve, add_every_n
    (3, 6, 1, False, False, False, 0.0, 1),       # 6 chains: less than a wave
    (6, 8, 4, True, False, False, 0.0, 2),        # general bounds / prior
    (30, 5, 64, False, False, False, 0.0, 1),     # DP = 32: the permuted row_pos; 320 chains: two pack chunks, the second partial
    (70, 4, 2, False, False, False, 0.0, 1),      # DP = 128: dimensions d + 64 e
    (16, 9, 5, False, False, False, 0.03, 3),     # evolving ladder
    (5, 7, 3, False, True, False, 0.0, 1),        # around a host-callback likelihood: unpack -> propose pass -> host llike -> accept pass
    (5, 7, 3, False, True, True, 0.0, 1),         # ... and a host prior callback
    (12, 6, 2, False, False, False, 0.02, 1),
]


@pytest.mark.parametrize("D,Nt,W,general,cb,prior_cb,ev,N", CASES)
def test_scripted_device_proposals_bit_exact(example, D, Nt, W, general, cb, prior_cb, ev, N):
    cap = 96
    pr, eng, lad, la = make_pair(example, D, Nt, W, general, cb, prior_cb, ev, N, cap=cap)
    assert eng.sweep_kernel_name.startswith("sweep_lanes_kernel<%d" % dp_of(D)), eng.sweep_kernel_name
    PU.assert_same_state(eng, lad, "start")
    nsteps = 30
    for k in range(nsteps):
        eng.step(1); eng.sync(); lad.pt_step(1)
        PU.assert_same_state(eng, lad, "after step %d" % (k + 1))
        check_outcome(eng, lad, la)
    assert la.user.calls == nsteps and la.user.result_calls == nsteps
    if ev:
        assert np.array_equal(eng.invtemps(), lad.betaw)
    acc, tries = int(eng.naccept.sum()) - eng.Nc, int(eng.ntries.sum()) - eng.Nc
    print("accepted %d of %d tries" % (acc, tries))
    assert 0 < acc < tries, (acc, tries)
    assert {0, 1, 2, 3, 4} <= set(eng.history()["last_type"].ravel().tolist())   # all five type codes (and -1: the initial rows)
    PU.assert_same_history_and_map(eng, lad, cap)
    eng.close()


# ------------------------------------------------------------------------------------------------------------- 3. count edges
def test_count_is_every_chain_without_an_exchange_phase(example):
    D, Nt, W = 4, 5, 3
    pr, eng, lad, la = make_pair(example, D, Nt, W, cap=0)
    for k in range(3):
        eng.sweep(1); eng.sync(); lad.sweep(1)
        n, r, w, a = la.outcome()
        assert n == eng.Nc and np.array_equal(r.astype(np.int64) * W + w, np.arange(eng.Nc))
        PU.assert_same_state(eng, lad, "after sweep %d" % (k + 1))
    assert la.user.calls == 3
    eng.close()


def test_count_zero_when_every_rung_was_touched(example):
    """two rungs at swap_rate 1: a step that tries the pair leaves no chain to move -- the launchers still run, nothing changes"""
    D, Nt, W = 4, 2, 2
    pr, eng, lad, la = make_pair(example, D, Nt, W, sr=1.0, cap=0)
    tried_steps = 0
    for k in range(16):
        before = eng.states()
        eng.step(1); eng.sync(); lad.pt_step(1)
        PU.assert_same_state(eng, lad, "after step %d" % (k + 1))
        pairs, acc = eng.last_swaps()
        n = check_outcome(eng, lad, la)
        assert la.user.calls == k + 1 and la.user.result_calls == k + 1
        if (pairs >= 0).any(axis=1).all():      # every ladder tried its one pair: both rungs touched everywhere
            tried_steps += 1
            assert n == 0
            if not acc.any():
                assert np.array_equal(eng.states(), before)
    assert tried_steps >= 1
    eng.close()


# -------------------------------------------------------------------------------------------------------------- 6. walker split
def test_device_proposals_name_the_global_walker_in_a_population_split(example):
    D, Nt, W, sr = 6, 5, 8, 0.3
    pr = GaussianProblem(D, Nt, 1e3)
    scale = scale_for(pr, D)
    rng = np.random.default_rng(11)
    x0 = (rng.uniform(-1.0, 1.0, size=(Nt * W, D)) * np.sqrt(np.diag(pr.cov))).reshape(Nt, W, D)

    def run(w0, n):
        eng = E.Engine(D, Nt, n, seed=SEED, swap_rate=sr, walker_begin=w0)
        pr.configure(eng, E.PROP_DIAG)
        la = Launcher(example, scale, Nt * n)
        la.attach(eng)
        eng.set_states(x0[:, w0:w0 + n].reshape(Nt * n, D))
        eng.step(12); eng.sync()
        cnt, r, w, a = la.outcome()
        assert cnt > 0 and w.min() >= w0 and w.max() < w0 + n and w.max() > w0
        out = eng.states().reshape(Nt, n, D), eng.llike.reshape(Nt, n), eng.naccept.reshape(Nt, n)
        eng.close()
        return out

    whole = run(0, W)
    lo, hi = run(0, W // 2), run(W // 2, W // 2)
    assert int(whole[2].sum()) > Nt * W       # moves were accepted
    for k in range(3):
        assert np.array_equal(whole[k][:, :W // 2], lo[k]) and np.array_equal(whole[k][:, W // 2:], hi[k]), k


# ------------------------------------------------------------------------------------------------------------------ 7. contract
def test_contract(example):
    D, Nt, W = 4, 8, 2
    pr = GaussianProblem(D, Nt, 1e2)
    scale = scale_for(pr, D)
    # refusals: part of a shard, a rung shard's step
    sh = E.Engine(D, Nt, W, rung_begin=0, rung_count=4)
    pr.configure(sh, E.PROP_DIAG)
    sh.init_from_prior()
    la = Launcher(example, scale, 4 * W)
    la.attach(sh)
    with pytest.raises(E.PtmError, match="ptm error -2.*partial sweeps"):
        sh.sweep_rungs(0, 2, True)
    with pytest.raises(E.PtmError, match="ptm error -2"):
        sh.exchange_finish_and_sweep(None, None)
    assert la.user.calls == 0
    sh.close()

    eng = E.Engine(D, Nt, W, seed=SEED, swap_rate=0.3)
    pr.configure(eng, E.PROP_DIAG)
    eng.init_from_prior()
    la = Launcher(example, scale, Nt * W)
    # the other proposal setters answer as they do with host-side proposals
    host_calls = []

    def host_fn(X, r, w, s):
        host_calls.append(s)
        return X, np.zeros(len(X)), np.zeros(len(X), dtype=np.int32), np.ones(len(X), dtype=np.int32)
    eng.set_proposal_callback(host_fn)
    with pytest.raises(E.PtmError) as host_answer:
        eng.set_proposal_de(0.1, 0.3, 4.0, 0.0)
    la.attach(eng)
    with pytest.raises(E.PtmError) as dev_answer:
        eng.set_proposal_de(0.1, 0.3, 4.0, 0.0)
    assert str(dev_answer.value) == str(host_answer.value)
    with pytest.raises(E.PtmError):
        eng.set_proposal_prior_draw(0)
    # the last proposal setter wins: device proposals cleared the host's ...
    eng.step(2); eng.sync()
    assert la.user.calls == 2 and not host_calls
    # ... and the reverse
    eng.set_proposal_callback(host_fn)
    eng.step(2); eng.sync()
    assert la.user.calls == 2 and len(host_calls) == 2
    la.attach(eng)
    eng.step(1); eng.sync()
    assert la.user.calls == 3 and len(host_calls) == 2
    # a bad argument (a result function without a propose function) leaves the setting in force
    with pytest.raises(E.PtmError, match="ptm error -1"):
        eng.set_proposal_device_c(None, la.result, user=C.addressof(la.user))
    eng.step(1); eng.sync()
    assert la.user.calls == 4
    assert eng.sweep_kernel_name.startswith("sweep_lanes_kernel<4")
    # back to the engine's own proposals
    eng.set_proposal_device(None)
    x1 = eng.states()
    eng.step(2); eng.sync()
    assert la.user.calls == 4 and len(host_calls) == 2
    assert not np.array_equal(eng.states(), x1)
    eng.close()


# --------------------------------------------------------------------------------------------------------- 8. late in a run
def test_late_in_a_run(example):
    """PT step 2^32 - 2 (tests/aging_util.py): step(3) in one call hands the launcher 2^32 - 2, 2^32 - 1, 2^32"""
    import aging_util as AU
    D, Nt, W, cap = 6, 6, 3, 32
    pr, eng, lad, la = make_pair(example, D, Nt, W, N=1, cap=cap)
    eng.step(4); eng.sync(); lad.pt_step(4)
    PU.assert_same_state(eng, lad, "before aging")
    view, shift = AU.age_pair(eng, lad, 3, step=AU.LATE_STEP)
    la.attach(eng)
    PU.assert_same_state(view, lad, "aged")
    eng.step(3); eng.sync(); lad.pt_step(3)
    calls = int(la.user.calls)
    assert calls == 7
    assert [int(la.user.last_step[(calls - 3 + i) % 4]) for i in range(3)] == [2**32 - 2, 2**32 - 1, 2**32]
    assert eng.step_count == lad.step == 2**32 + 1
    PU.assert_same_state(view, lad, "after crossing 2^32")
    check_outcome(eng, lad, la)
    eng.close()


# ------------------------------------------------------------------------------------------------- 4, 5. the torch cases
def _worker(case, *args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(HERE, "device_proposal_worker.py"), case, json.dumps(list(args))],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and ("OK " + case) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_device_proposals_with_a_device_likelihood():
    _worker("devlike", 6, 7, 5)


def test_torch_binding():
    _worker("torch_binding", 5, 6, 4)


# ------------------------------------------------------------------------------------------------------------------ 9. facade
def test_facade_device_proposal_with_device_likelihood(tmp_path):
    d = str(tmp_path)
    exe = os.path.join(d, "device_proposal")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), "-x", "hip", os.path.join(HERE, "cxx", "device_proposal_main.cc"),
                           os.path.join(ROOT, "examples", "scripted_device_proposal.hip"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
                           "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-o", exe])
    lines = {}
    for mode in ("1", "0"):
        env = dict(os.environ, PTM_DEVICE_PROPOSAL=mode)
        r = subprocess.run([exe, "run" + mode], capture_output=True, text=True, timeout=600, cwd=d, env=env)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines[mode] = [l for l in r.stdout.splitlines() if "proposal" in l and "path" in l]
        assert lines[mode], r.stdout[-3000:]
    files = sorted(f for f in os.listdir(d) if f.startswith("run1") and f.endswith(".dat"))
    assert files, os.listdir(d)
    for f in files:
        a = open(os.path.join(d, f), "rb").read()
        b = open(os.path.join(d, "run0" + f[4:]), "rb").read()
        assert len(a) > 1000 and a == b, f
    assert lines["1"] != lines["0"], lines
