"""Child process of tests/test_gpu_device_proposals.py: the cases of device proposals (ptm_set_proposal_device) that need torch --
a torch device likelihood beside them, and proposals written as a torch function (Engine.set_proposal_device).

torch is imported FIRST (tests/torch_shard_worker.py says why: one HIP runtime per process).  Usage: device_proposal_worker.py CASE [ARGS..];
prints "OK <case>" on success, raises (non-zero exit) otherwise."""
import json
import math
import os
import sys
import tempfile

import torch  # noqa: E402  (before anything loads libptm_engine.so)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np

import oracle_lib as O
import parity_util as PU
import test_gpu_device_proposals as T
from ptmcmc_amd import engine as E
from ptmcmc_amd.problems import GaussianProblem
from test_gpu_host_proposals import scripted_proposal

DEV = torch.device("cuda", 0)


def _same(a, b, what):
    for name in ("llike", "lprior", "ntries", "naccept", "last_type", "nhist"):
        u, v = getattr(a, name), getattr(b, name)
        assert np.array_equal(u, v, equal_nan=True), (what, name, np.argwhere(u != v)[:4].tolist())
    assert np.array_equal(a.states(), b.states()), what


# ------------------------------------------------------------------------------------- device proposals + device likelihood
def case_devlike(D, Nt, W):
    """the same diagonal quadratic as a torch device likelihood, as a host-callback likelihood and in the checker, under the HIP
    launcher's proposals (the checker: their numpy twin): three identical runs.  D < 8, so numpy's sum adds in index order, as the
    torch loop does; every other operation is one exactly rounded product."""
    assert D < 8
    sc = [float(v) for v in np.linspace(0.7, 1.4, D)]
    ll_numpy = T.diag_loglike(D)
    rec = {"on": True, "b": []}

    def ll_torch(X, count, out):
        acc = None
        for d in range(D):
            t = X[:, d] * sc[d]
            t = t * t
            acc = t if acc is None else acc + t
        out.copy_(acc * (-0.5))
        if rec["on"]:
            rec["b"].append((X.clone(), count.clone(), out.clone()))

    with tempfile.TemporaryDirectory() as d:
        lib = T.build_example(d)
        pr = GaussianProblem(D, Nt, 1e3)
        scale = T.scale_for(pr, D)
        rng = np.random.default_rng(5)
        x0 = rng.uniform(-1.0, 1.0, size=(Nt * W, D)) * np.sqrt(np.diag(pr.cov))
        engines, launchers = [], []
        for target in ("device", "host"):
            eng = E.Engine(D, Nt, W, seed=T.SEED, swap_rate=0.35)
            pr.configure(eng, E.PROP_DIAG)
            la = T.Launcher(lib, scale, Nt * W)
            if target == "device":      # either order of the two setters works: here the proposals first ...
                la.attach(eng)
                eng.set_target_device(ll_torch)
            else:
                eng.set_target_callback(ll_numpy)
                la.attach(eng)
            engines.append(eng); launchers.append(la)
        dev, host = engines
        assert dev.step_kernel_name.endswith(" + device likelihood"), dev.step_kernel_name
        assert dev.sweep_kernel_name.startswith("sweep_lanes_kernel<8"), dev.sweep_kernel_name
        rec["b"].clear()
        dev.set_states(x0); host.set_states(x0)
        pb = PU.oracle_problem(pr)
        pb.set_user(ll_numpy)
        lad = O.Ladder(pb, pr.beta, W=W, swap_rate=0.35)
        lad.set_proposals([(O.PROP_DIAG, np.ones(D), 0.0)] * Nt)
        lad.use_philox(T.SEED)
        cfn = O.make_propose_fn(scripted_proposal(scale))
        lad.set_host_proposal(cfn)
        lad.set_states(PU.to_oracle_order(x0, Nt, W))
        PU.assert_same_state(dev, lad, "start (device likelihood)")
        PU.assert_same_state(host, lad, "start (host likelihood)")
        for s in range(6):
            dev.step(5); host.step(5)      # (the device engine's five steps are queued before anything waits)
            dev.sync(); host.sync(); lad.pt_step(5)
            what = "after %d steps" % (5 * (s + 1))
            PU.assert_same_state(dev, lad, what + " (device likelihood)")
            PU.assert_same_state(host, lad, what + " (host likelihood)")
            T.check_outcome(dev, lad, launchers[0])
            T.check_outcome(host, lad, launchers[1])
        assert launchers[0].user.calls == 30 and launchers[1].user.calls == 30
        acc, tries = int(dev.naccept.sum()) - dev.Nc, int(dev.ntries.sum()) - dev.Nc
        assert 0 < acc < tries, (acc, tries)
        # best_evaluated: the maximum of lprior + llike over every row the likelihood was asked to evaluate
        rec["on"] = False
        best_v, best_x = -math.inf, None
        for X, cnt, out in rec["b"]:
            n = int(cnt.item())
            assert X.shape[0] == dev.Nc
            if n == 0:
                continue
            Xn = X[:n].cpu().numpy()
            post = dev.debug_evaluate(Xn)[2] + out[:n].cpu().numpy()
            j = int(np.nanargmax(np.where(np.isnan(post), -np.inf, post)))
            if post[j] > best_v:
                best_v, best_x = post[j], Xn[j]
        got_v, got_x = dev.best_evaluated()
        assert got_v == best_v, (got_v, best_v)
        assert np.array_equal(got_x, best_x)
        dev.close(); host.close()


# ----------------------------------------------------------------------------------------------------------- the torch binding
def case_torch_binding(D, Nt, W):
    """a proposal written in torch (+, *, integer operations, where) against the same function in numpy as a host callback: a
    reflection about a per-rung centre with a scripted log-Hastings ratio, type and validity"""
    pr = GaussianProblem(D, Nt, 1e2)
    sig = np.sqrt(np.diag(pr.cov))
    centre2 = np.ascontiguousarray(np.linspace(-0.4, 0.6, Nt)[:, None] * sig[None, :] * 2.0)      # twice the centre of each rung
    centre2_t = torch.as_tensor(centre2, device=DEV)
    seen = {"calls": 0, "results": 0}

    def propose_torch(X, rung, walker, count, step, P, H, Tt, V):
        seen["calls"] += 1
        r = rung.to(torch.int64)
        P.copy_(X * (-1.0) + centre2_t[r])
        k = rung * 7 + walker * 3 + step
        H.copy_((k % 5).to(torch.float64) * 0.25 + (-0.5))
        Tt.copy_((rung + walker) % 3)
        V.copy_(torch.where((walker + step) % 11 == 0, torch.zeros_like(V), torch.ones_like(V)))

    acc_sum = torch.zeros(1, dtype=torch.int64, device=DEV)

    def result_torch(rung, walker, count, accepted):
        seen["results"] += 1
        live = torch.arange(accepted.shape[0], device=DEV) < count
        acc_sum.add_(torch.where(live, accepted, torch.zeros_like(accepted)).sum())

    host_acc = {"n": 0}

    def propose_numpy(X, rung, walker, step):
        P = X * (-1.0) + centre2[rung]
        k = rung * 7 + walker * 3 + step
        H = (k % 5).astype(np.float64) * 0.25 + (-0.5)
        Tn = ((rung + walker) % 3).astype(np.int32)
        V = np.where((walker + step) % 11 == 0, 0, 1).astype(np.int32)
        return P, H, Tn, V

    def result_numpy(rung, walker, accepted):
        host_acc["n"] += int(accepted.sum())

    rng = np.random.default_rng(3)
    x0 = rng.uniform(-1.0, 1.0, size=(Nt * W, D)) * sig
    dev = E.Engine(D, Nt, W, seed=T.SEED, swap_rate=0.3)
    host = E.Engine(D, Nt, W, seed=T.SEED, swap_rate=0.3)
    for eng in (dev, host):
        pr.configure(eng, E.PROP_DIAG)
    dev.set_proposal_device(propose_torch, result=result_torch)
    host.set_proposal_callback(propose_numpy, result=result_numpy)
    dev.set_states(x0); host.set_states(x0)
    assert dev.sweep_kernel_name.startswith("sweep_lanes_kernel<8"), dev.sweep_kernel_name
    _same(dev, host, "start")
    for s in range(3):
        dev.step(10)
        assert seen["calls"] == 10 * (s + 1) and seen["results"] == 10 * (s + 1)      # queued: called before anything waited
        host.step(10); dev.sync(); host.sync()
        _same(dev, host, "after %d steps" % (10 * (s + 1)))
    acc, tries = int(dev.naccept.sum()) - dev.Nc, int(dev.ntries.sum()) - dev.Nc
    assert 0 < acc < tries, (acc, tries)
    assert int(acc_sum.item()) == host_acc["n"] == acc
    assert set(np.unique(dev.last_type).tolist()) >= {0, 1, 2}
    # None switches the device proposals off: the engine's own set runs
    dev.set_proposal_device(None)
    dev.step(2); dev.sync()
    assert seen["calls"] == 30
    dev.close(); host.close()


CASES = {"devlike": case_devlike, "torch_binding": case_torch_binding}

if __name__ == "__main__":
    torch.cuda.init()
    name, args = sys.argv[1], json.loads(sys.argv[2]) if len(sys.argv) > 2 else []
    CASES[name](*args)
    print("OK", name, args, flush=True)
