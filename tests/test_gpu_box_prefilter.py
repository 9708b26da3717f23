"""The box pre-pass of big-population steps (ptmcmc_amd/csrc/ptm_box_prefilter.hpp): a kernel in front of the compacted 32-dimension
sweep that settles the chains whose proposal has left the uniform prior's box in its first 16 dimensions.  It changes which kernel
does the work and nothing in the chains: every case runs engine against oracle bit for bit (tests/box_prefilter_worker.py), in a
process of its own because PTM_BOX_PREFILTER is read once per process.  12 rungs x 1024 walkers in 32 dimensions is the smallest
shape that engages the compacted sweep; its ladder (beta = 1, 0.15, 0.023, 3.5e-3, 5.3e-4, 8e-5, ...) has four cold rungs deep
inside the box, one in between and seven hot ones, where a CPU model of the sampler puts ~0.65 of the proposals outside the box in
dimensions 0..15 (~0.43 over all twelve rungs)."""
import functools
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def run(case, setting):
    """one worker run (cached: the counters of a run serve several tests); setting: PTM_BOX_PREFILTER's value, None: unset"""
    env = dict(os.environ)
    env.pop("PTM_BOX_PREFILTER", None)
    if setting is not None:
        env["PTM_BOX_PREFILTER"] = setting
    r = subprocess.run([sys.executable, os.path.join(HERE, "box_prefilter_worker.py"), case], env=env, capture_output=True, text=True, timeout=120)   # (a worker takes about a second: the limit only ends a hung one)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-3000:]
    out = dict(kv.split("=") for kv in r.stdout.split()[1:])
    print(case, setting, out)
    return {k: int(v) for k, v in out.items()}


def test_forced_prepass_matches_the_oracle_and_settles_a_fair_share():
    """PTM_BOX_PREFILTER=1: every rung goes through the pre-pass.  3 + 4 + 5 PT steps with plain sweeps and a checkpoint / resume in
    between, states (through the row labels: eng.states() runs restore_rows_kernel), llikes, lpriors, counters and swap counts
    equal to the oracle's after each leg; the pre-pass ran and settled between 0.2 and 0.9 of what it saw -- neither outcome absent."""
    c = run("lower", "1")
    assert c["eligible"] == 1 and c["rungs_flagged"] == c["rungs"] == 12
    assert c["seen"] > 0 and c["accepts"] > 0
    assert 0.2 * c["seen"] < c["settled"] < 0.9 * c["seen"], c


def test_automatic_prepass_takes_the_hot_rungs_only():
    """unset: the host's estimate flags the rungs whose proposals are as wide as the box and leaves the cold ones to the sweep alone"""
    c, forced = run("lower", None), run("lower", "1")
    assert c["eligible"] == 1 and 0 < c["rungs_flagged"] < c["rungs"], c
    assert 0 < c["seen"] < forced["seen"], (c, forced)
    assert c["accepts"] == forced["accepts"]


def test_prepass_switched_off():
    c = run("lower", "0")
    assert c["seen"] == 0 and c["settled"] == 0 and c["rungs_flagged"] == 0 and c["eligible"] == 0
    assert c["accepts"] == run("lower", "1")["accepts"]


def test_dense_factor_never_engages_the_prepass():
    """a dense (eigenvector) factor reaches every row from every column: the first 16 coordinates need all 32 normals"""
    c = run("dense", "1")
    assert c["seen"] == 0 and c["settled"] == 0 and c["eligible"] == 0, c


def test_chains_without_a_finite_posterior_reach_the_sweep():
    """300 chains start outside the prior box (lprior = -inf): the reference accepts their moves whatever the proposal is (a NaN
    log-Hastings ratio stays accepted), so the pre-pass may not settle them even when its box test fails"""
    c = run("nonfinite", "1")
    # the 300 chains are really outside, spread over every rung, and every rung goes through the pre-pass: the case cannot be vacuous
    assert c["outside"] == 300 and c["outside_rungs"] == 12 and c["rungs_flagged"] == c["rungs"] == 12, c
    assert c["seen"] > 0 and 0 < c["settled"] < c["seen"], c


@pytest.mark.parametrize("overlap", [False, True])
def test_prepass_in_sharded_engines(overlap):
    """the pre-pass in front of the sharded step's partial sweeps (interior / boundary rungs separately): the shards' chains equal the
    whole-ladder engine's"""
    c = run("sharded_overlap" if overlap else "sharded", "1")
    assert c["eligible"] == 1 and c["rungs_flagged"] == c["rungs"] == 24
    assert 0 < c["settled"] < c["seen"], c
