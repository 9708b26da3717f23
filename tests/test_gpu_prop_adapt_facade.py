"""The facade's proposal adaptation (tests/cxx/prop_adapt_device_main.cc): parallel_tempering_chains::adapt_gaussian_proposals on the
device (ptm_adapt_proposals) and by its host route (PTM_HOST_PROPOSAL_ADAPT=1: posterior_moments, gaussian_prop::eigen_factor,
ptm_set_proposal_rung) write the same chain files.  The sampler's --prop_cov_adapt_every (tests/cxx/prop_adapt_sampler_main.cc) prints
its line at every adaptation, stops adapting at burn_frac * nsteps, and without the flag writes what a run that never adapts writes."""
import glob
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ptmcmc_amd", "host"), "-L", os.path.join(ROOT, "ptmcmc_amd"), "-lptm_engine",
         "-Wl,-rpath," + os.path.join(ROOT, "ptmcmc_amd"), "-pthread"]
LINE = re.compile(r"^Proposal factors from (\d+) rows x (\d+) replicas: (\d+) of (\d+) rungs set, (\d+) kept \(not finite\), (\d+) kept \(not positive definite\) \((device|host)\) at step (\d+)$")

pytestmark = pytest.mark.gpu


def build(d, name, source):
    exe = os.path.join(d, name)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "cxx", source)] + FLAGS + ["-o", exe])
    return exe


def run(exe, args, host=False):
    env = dict(os.environ)
    env.pop("PTM_HOST_PROPOSAL_ADAPT", None)
    if host:
        env["PTM_HOST_PROPOSAL_ADAPT"] = "1"
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def files(d, base):
    got = {os.path.basename(p)[len(base):]: open(p).read() for p in sorted(glob.glob(os.path.join(d, base + "*.dat")))}
    assert got and all(len(v) > 1000 for v in got.values()), list(got)
    return got


@pytest.fixture(scope="module")
def device_exe():
    with tempfile.TemporaryDirectory() as d:
        yield build(d, "propadaptdev", "prop_adapt_device_main.cc"), d


@pytest.fixture(scope="module")
def sampler():
    with tempfile.TemporaryDirectory() as d:
        yield build(d, "propadaptsampler", "prop_adapt_sampler_main.cc"), d


@pytest.mark.parametrize("kind", ["dense", "diag"])
def test_device_route_and_host_route_write_the_same_chain_files(device_exe, kind):
    exe, d = device_exe
    dev = run(exe, [os.path.join(d, kind + "_dev"), kind])
    host = run(exe, [os.path.join(d, kind + "_host"), kind], host=True)
    a_dev, a_host = ([l for l in out if l.startswith("adapt")] for out in (dev, host))
    print(a_dev, a_host)
    assert len(a_dev) == 2 and all(l.endswith("device=1") for l in a_dev) and all(l.endswith("device=0") for l in a_host)
    assert [l.rsplit(" ", 1)[0] for l in a_dev] == [l.rsplit(" ", 1)[0] for l in a_host]
    assert a_dev[0].startswith("adapt rows=150 rungs=4 set=4 ") and a_dev[1].startswith("adapt rows=400 rungs=4 set=4 ")
    f_dev, f_host = files(d, kind + "_dev"), files(d, kind + "_host")
    assert len(f_dev) == 4 and f_dev == f_host


def test_host_side_proposals_are_left_alone_and_say_so_once(device_exe):
    exe, d = device_exe
    out = run(exe, [os.path.join(d, "hp"), "hostprop"])
    assert len([l for l in out if "adapt_gaussian_proposals: nothing is adapted" in l]) == 1
    assert [l for l in out if l.startswith("adapt")] == ["adapt rows=0 rungs=0 set=0 not_finite=0 not_positive=0 device=0"] * 2


def test_sampler_adapts_during_burn_in_only_and_both_routes_write_the_same_chain_files(sampler):
    exe, d = sampler
    dev = run(exe, [os.path.join(d, "ad"), "--prop_cov_adapt_every=200"])
    host = run(exe, [os.path.join(d, "ah"), "--prop_cov_adapt_every=200"], host=True)
    lines = [LINE.match(l) for l in dev if l.startswith("Proposal factors")]
    assert all(lines) and [int(m.group(8)) for m in lines] == [200, 400, 600, 800]       # burn_frac 0.5 of 2000 steps: never at 1000 or after
    assert all(m.group(7) == "device" and m.group(1) == "100" and m.group(3) == m.group(4) == "6" for m in lines), [m.group(0) for m in lines]
    hl = [l for l in host if l.startswith("Proposal factors")]
    assert [l.replace("(host)", "(device)") for l in hl] == [m.group(0) for m in lines]
    assert files(d, "ad") == files(d, "ah")
    rows = run(exe, [os.path.join(d, "ar"), "--prop_cov_adapt_every=300", "--prop_cov_adapt_rows=40", "--prop_cov_adapt_scale=0.5", "--burn_frac=0.3"])
    lines = [LINE.match(l) for l in rows if l.startswith("Proposal factors")]
    assert [(int(m.group(8)), m.group(1)) for m in lines] == [(300, "40")]                # burn-in ends at step 600


def test_sampler_without_the_flag_writes_what_a_run_that_never_adapts_writes(sampler):
    exe, d = sampler
    plain = run(exe, [os.path.join(d, "pl")])
    never = run(exe, [os.path.join(d, "nv"), "--prop_cov_adapt_every=5000"])             # (its first multiple lies past the burn-in)
    cut = run(exe, [os.path.join(d, "ct"), "--prop_cov_adapt_every=200", "--burn_frac=0.05"])   # steps in pieces of 200 until step 100, adapts never
    adapted = run(exe, [os.path.join(d, "ad2"), "--prop_cov_adapt_every=200"])
    assert not any(l.startswith("Proposal factors") for l in plain + never + cut) and any(l.startswith("Proposal factors") for l in adapted)
    assert files(d, "pl") == files(d, "nv")
    assert files(d, "pl") != files(d, "ad2")                                              # ... and adapting does change the chains
