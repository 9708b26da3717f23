"""Differential evolution on the f64 matrix cores (de_mfma32_kernel, ptmcmc_amd/csrc/ptm_de_mfma_kernel.hpp): the 32-D sweep of a
population with whole waves per rung whose proposal set holds differential evolution.  Unset, PTM_DE_MFMA leaves the choice to the
population (chains x 32 > 2^21: where the lanes kernel used to hand over to sweep_kernel<32, ...>); the parity cases below are small,
so each runs with PTM_DE_MFMA=1 PTM_LADDER=0 in a process of its own (tests/de_mfma_worker.py: the engine reads its switches once) --
engine against oracle bit for bit: states, scalars, counters, every saved row, the MAPs.  The default routing is asserted in this
process, on a population just past the rule's edge."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def run(case):
    env = dict(os.environ)
    env["PTM_DE_MFMA"] = "1"
    env["PTM_LADDER"] = "0"
    r = subprocess.run([sys.executable, os.path.join(HERE, "de_mfma_worker.py"), case], env=env, capture_output=True, text=True, timeout=180)   # (a worker takes seconds: the limit only ends a hung one)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-3000:]
    out = dict(kv.split("=", 1) for kv in r.stdout.split()[1:])
    print(case, out)
    return out


@pytest.mark.parametrize("case,name", [
    ("one_wave", "de_mfma32_kernel<0,false>"),       # (32, 3, 64, DENSE): one wave per rung, no pad lane
    ("straddle", "de_mfma32_kernel<2,false>"),       # (21, 4, 320, LOWER, every second add): pad dimensions, tiles across rungs, six Gaussians
    ("snooker_diag", "de_mfma32_kernel<2,false>"),   # (17, 2, 128, DIAG): snooker moves only, a diagonal factor as a Cholesky factor
    ("parallel", "de_mfma32_kernel<2,false>"),       # (20, 3, 64, LOWER): parallel moves only
    ("no_init", "de_mfma32_kernel<2,false>"),        # (17, 2, 64, LOWER), 200 steps: passed over until 170 rows are saved, then drawn
    ("evolving", "de_mfma32_kernel<0,true>"),        # (32, 6, 64, DENSE), evolving ladders: the temperatures are the oracle's too
    ("limit_mean", "de_mfma32_kernel<2,false>"),     # (24, 3, 64, LOWER): limit bounds on four dimensions and a target mean
])
def test_differential_evolution_on_the_matrix_cores_matches_the_oracle(case, name):
    """member choice and the passing-over of a differential evolution that is not ready, row picks from the initial rows and from the
    ring, parallel and snooker moves formed on the matrix lanes, the snooker move's log-Hastings ratio, type codes: after 1, 4 and the
    remaining PT steps bit for bit the oracle's; differential-evolution and Gaussian types were both accepted (the worker asserts)"""
    out = run(case)
    assert out["kernel"] == name and int(out["accepts"]) > 0, out


def test_plain_sweeps_and_sweeps_over_rung_ranges():
    """ptm_sweep and ptm_sweep_rungs (two ranges a step, the second closing it) go through the same kernel, honouring the range"""
    assert run("sweeps")["kernel"] == "de_mfma32_kernel<2,false>"


def test_a_history_ring_too_short_is_reported_from_this_kernel():
    assert run("short_ring")["error"] == "history"


def test_the_general_state_space_stays_on_the_general_kernels():
    """wrap bounds, a Gaussian prior factor: the switch on, and still the lanes kernel (or sweep_kernel<32, ...)"""
    for n in run("name_gen2")["kernel"].split("|"):
        assert n.startswith("sweep_lanes_kernel<") or n.startswith("sweep_kernel<32"), n


def test_a_prior_draw_member_stays_on_the_general_kernels():
    n = run("name_prior_draw")["kernel"]
    assert n.startswith("sweep_lanes_kernel<") or n.startswith("sweep_kernel<32"), n


def test_a_big_population_goes_to_the_matrix_cores_by_default():
    """No switch: 2 rungs x 32832 walkers = 65664 chains x 32 padded dimensions is just past 2^21 lanes, where differential evolution
    used to leave the lanes kernel for sweep_kernel<32, ...>.  Nothing is saved yet (no initial rows), so the member is passed over
    and every chain takes a Gaussian: 257 tiles of the kernel against the oracle for three PT steps."""
    import parity_util as PU
    from ptmcmc_amd import engine as E
    from proposal_pairs import de_pair
    assert "PTM_DE_MFMA" not in os.environ and "PTM_FORCE_VALU" not in os.environ
    pr, eng, lad = de_pair(32, 2, 32832, E.PROP_LOWER, 1, 0.3, 0, 2, 8)
    assert eng.sweep_kernel_name.startswith("de_mfma32_kernel<"), eng.sweep_kernel_name
    assert eng.step_kernel_name == "decide_kernel + de_mfma32_kernel<2, false>", eng.step_kernel_name
    eng.step(3); eng.sync(); lad.pt_step(3)
    PU.assert_same_state(eng, lad, "after 3 PT steps")
    lt = eng.last_type   # (-1: nothing accepted yet; member 0 is the differential evolution)
    assert (lt >= 1).any() and not (lt[lt >= 0] % 10 == 0).any(), np.unique(lt)
    eng.close()


@pytest.mark.parametrize("Nt,W", [(16, 320), (2, 64)])
def test_smaller_populations_keep_the_lanes_kernel_by_default(Nt, W):
    from ptmcmc_amd import engine as E
    from proposal_pairs import de_pair
    assert "PTM_DE_MFMA" not in os.environ
    pr, eng, lad = de_pair(32, Nt, W, E.PROP_LOWER, 1, 0.3, 0, 2, 8)
    assert eng.sweep_kernel_name.startswith("sweep_lanes_kernel<"), eng.sweep_kernel_name
    eng.close()
