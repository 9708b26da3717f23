"""User priors evaluated ON THE DEVICE (ptm_set_prior_device) beside a device likelihood: the engine packs the valid proposals, calls
the user's batched log-prior on its own stream, applies the reference's prior gate in a kernel, and goes on to the likelihood's pack
-- no host wait anywhere in the step.

Each case runs in a child process that imports torch first (tests/device_prior_worker.py; tests/torch_shard_worker.py says why), under
its own time limit.  Oracle parity uses torch functions whose bits equal the numpy forms the oracle calls (+ - * only, one
elementwise op per kernel, columns summed in a fixed order); the device-vs-host cases run the same torch functions both ways."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "device_prior_worker.py")


def _run(case, *args, timeout=600):
    r = subprocess.run([sys.executable, WORKER, case, json.dumps(list(args))], capture_output=True, text=True, timeout=timeout)
    if r.returncode < 0 or r.returncode in (134, 139):   # a crashed child (abort, fault): start nothing more on the device
        pytest.exit("device-prior worker %s%s died (exit %d)\n%s" % (case, list(args), r.returncode, r.stderr[-6000:]), returncode=1)
    assert r.returncode == 0 and ("OK %s" % case) in r.stdout, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-6000:])


@pytest.mark.parametrize("D,Nt,W,ev", [
    (3, 6, 4, 0.0),        # a partial wave
    (12, 8, 3, 0.02),      # evolving ladders: each chain has its own beta
    (6, 20, 13, 0.0),      # 260 chains: the second chunk of the pack holds 4
    (20, 5, 64, 0.0),      # whole waves per rung: the general kernel
    (40, 6, 3, 0.0),       # the lanes kernel
])
def test_device_prior_matches_the_oracle(D, Nt, W, ev):
    """the prior of test_host_evaluated_prior_matches_the_oracle (a correlated Gaussian times a hard disc; wrap and limit bounds) on the
    device, bit for bit against the oracle at the start and after each of 6 x 5 steps; the prior never sees an invalid state, the
    likelihood never one outside the disc, and the prior does see states outside the disc"""
    _run("oracle", D, Nt, W, ev)


def test_empty_batches():
    """every proposal invalid (limit bounds of width 1, proposal sigma 1e6): both functions are called with count 0 in every step, no
    state moves, the chain is the oracle's"""
    _run("empty")


@pytest.mark.parametrize("ev,de", [(0.0, False), (0.02, False), (0.0, True), (0.02, True)])
def test_device_path_equals_host_path_with_transcendental_functions(ev, de):
    """the same torch prior (cos, exp, a hard cut) and toy-LISA likelihood through set_prior_device + set_target_device and through
    set_prior_callback + set_target_callback: equal chains, history rings and MAPs"""
    _run("vs_host", 20, 4, ev, de)


def test_device_prior_beside_device_proposals():
    """scripted proposals on the device + device prior + device likelihood against the oracle: the whole step stays on the device"""
    _run("devprop", 5, 7, 3)


def test_state_set_up_and_best_use_the_device_prior():
    """set_states without llike against the oracle, debug_evaluate's log-priors, best_evaluated = max of lprior + llike over the rows
    the likelihood saw with the prior's recorded values, ptm_restore"""
    _run("setup_best")


def test_device_prior_contract():
    """200 steps queued before anything waits, n_rows = local chains; every refusal is -2 and the engine steps on; set_prior_device(None)
    gives the chain of an engine that never had one; the setters' order is free"""
    _run("contract")


def test_hip_example_prior():
    """examples/correlated_prior_device.hip built here: the kernel against its host form on 10^4 in-prior states (equal bits);
    examples/example_lisa_device_prior.cc writes the same chain files with PTM_DEVICE_PRIOR=1 and =0, and names the device prior in
    its kernel line on the device route"""
    _run("hip_example", timeout=1200)
