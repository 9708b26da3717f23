"""User likelihoods evaluated ON THE DEVICE (ptm_set_target_device): the engine calls the user's batched function on its own stream
between the propose pass and the accept pass (pack -> the user's work -> scatter), with no host wait.

Each case runs in a child process that imports torch first (tests/device_like_worker.py; tests/torch_shard_worker.py says why), under
its own time limit.  Oracle parity uses a torch polynomial whose bits equal the numpy form the oracle calls (+ - * only, one
elementwise op per kernel, columns summed in a fixed order); the device-vs-host cases run the same torch toy-LISA function both ways."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "device_like_worker.py")


def _run(case, *args, timeout=600):
    r = subprocess.run([sys.executable, WORKER, case, json.dumps(list(args))], capture_output=True, text=True, timeout=timeout)
    if r.returncode < 0 or r.returncode in (134, 139):   # a crashed child (abort, fault): start nothing more on the device
        pytest.exit("device-likelihood worker %s%s died (exit %d)\n%s" % (case, list(args), r.returncode, r.stderr[-6000:]), returncode=1)
    assert r.returncode == 0 and ("OK %s" % case) in r.stdout, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-6000:])


@pytest.mark.parametrize("Nt,W", [(16, 4), (128, 1)])
@pytest.mark.parametrize("ev", [0.0, 0.02])
def test_device_likelihood_matches_the_oracle_C5_shape(Nt, W, ev):
    """BASELINE configs[4]'s shapes: mixed uniform/polar/copolar prior, wrap and limit bounds, fixed and evolving ladder"""
    _run("c5", Nt, W, ev)


@pytest.mark.parametrize("Nt,W", [(20, 1), (16, 64)])
def test_device_likelihood_with_the_default_recipe_matches_the_oracle(Nt, W):
    """differential evolution (0.8) + Gaussians drawn on the device, evolving ladder, history and MAP"""
    _run("recipe", 6, Nt, W, 1, 40, 0.01, 0.8, 4, 10)


@pytest.mark.parametrize("D", [12, 40, 140])
def test_device_likelihood_through_the_lanes_kernel(D):
    _run("lanes", D, 4 if D > 40 else 6, 3, 0.02 if D == 40 else 0.0)


def test_device_likelihood_through_the_general_kernel_whole_waves():
    _run("general")


def test_device_likelihood_with_minus_inf_and_nan_regions_matches_the_oracle():
    """a likelihood that is -inf and NaN in parts of the space: rejections (and NaN acceptances) as the oracle makes them"""
    _run("c5", 16, 4, 0.0, True)


@pytest.mark.parametrize("ev,de", [(0.0, False), (0.02, False), (0.0, True), (0.02, True)])
def test_device_path_equals_host_path_with_transcendental_functions(ev, de):
    _run("vs_host", 20, 4, ev, de)


def test_state_set_up_uses_the_device_likelihood():
    """set_states without llike, init_from_prior_k with redraws, draw_prior_rows, debug_evaluate"""
    _run("setup")


@pytest.mark.parametrize("Nt,W,ev", [(20, 1, 0.0), (16, 64, 0.01)])
def test_best_evaluated_is_the_maximum_over_the_evaluated_rows(Nt, W, ev):
    _run("best", Nt, W, ev)


def test_device_likelihood_contract():
    """once per sweep with n_rows = local chains; step(200) queues without waiting; refusals; the last target setter wins"""
    _run("contract")


def test_hip_example_likelihood():
    """examples/lisa_device_likelihood.hip built here: its llikes against lisa_toy.loglike (1e-12 relative); an engine driven by its
    launcher through set_target_device_c equals one whose host callback round-trips it; examples/example_lisa_device.cc writes the
    same chain files on the device path and the host path (PTM_DEVICE_LIKE=0), and best_post agrees"""
    _run("hip_example", timeout=1200)
